#!/usr/bin/env python3
"""A dictionary per file, S files at once: the dictionary set (tries built on the device, one launch per kernel for all
sequences) against S x the per-dictionary path (crgpu_dict_create + crgpu_dict_*_blocks_dev), measured in one process on
one device, the two orders alternating. python tools/dict_set_rate.py [--sizes 1,16,128] [--reps 5]

Files: enwik_like(1 MiB, seed s), s = 0 .. S-1, each with the dictionary the host dicpick picks for it, cut into 16 blocks
of 64 KiB. (a) create: wall clock of S crgpu_dict_create calls / of one crgpu_dict_set_create (both return with the
dictionaries ready on the device), and the set's kernel ms from the stage log. (b) stage: encode then decode of all S x 16
blocks from device memory, as S pairs of calls / as one pair; wall clock to the final synchronise, and kernel ms from the
stage log. Medians over the repetitions."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from comprox_amd import CrGpu, corpus

BLOCK, PER = 65536, 16
vp = ctypes.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,128")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    dev = torch.device("cuda", 0)
    g = CrGpu(0)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    L = g.lib
    files = [corpus.enwik_like(PER * BLOCK, s) for s in range(max(sizes))]
    texts = [bench.host_dicpick(L, f) for f in files]
    print(f"{len(files)} files of {PER * BLOCK} bytes; dictionary words min/median/max = "
          f"{min(t.count(10) for t in texts)}/{int(statistics.median(t.count(10) for t in texts))}/{max(t.count(10) for t in texts)}")
    g.stage_log(True)

    def kernel_ms():
        return sum(v[0] for v in g.stage_log_read().values())

    print("S | create: S x dict_create ms | dict_set_create ms (kernels ms) | stage: S pairs ms (kernels ms) | one pair ms (kernels ms) | nodes")
    for S in sizes:
        nb = S * PER
        d_in = torch.from_numpy(np.concatenate(files[:S])).to(dev)
        off = torch.arange(nb, dtype=torch.int64, device=dev) * BLOCK
        size = torch.full((nb,), BLOCK, dtype=torch.int32, device=dev)
        slot = (BLOCK + 1 + 63) // 64 * 64
        mid = torch.zeros(nb * slot, dtype=torch.uint8, device=dev)
        mid_off = torch.arange(nb, dtype=torch.int64, device=dev) * slot
        mid_len = torch.zeros(nb, dtype=torch.int32, device=dev)
        back = torch.zeros(nb * BLOCK, dtype=torch.uint8, device=dev)
        back_len = torch.zeros(nb, dtype=torch.int32, device=dev)
        seq_first = (np.arange(S + 1) * PER).astype(np.uint32)

        def create_each():
            return [g.dict_create(t) for t in texts[:S]]

        def create_set():
            return g.dict_set_create(texts[:S])

        def stage_each(ds):
            for s, d in enumerate(ds):
                o8, o4 = s * PER * 8, s * PER * 4
                rc = L.crgpu_dict_encode_blocks_dev(g.h, d.h, vp(d_in.data_ptr()), vp(off.data_ptr() + o8), vp(size.data_ptr() + o4), PER, BLOCK,
                                                    vp(mid.data_ptr()), vp(mid_off.data_ptr() + o8), vp(mid_len.data_ptr() + o4), 0)
                rc |= L.crgpu_dict_decode_blocks_dev(g.h, d.h, vp(mid.data_ptr()), vp(mid_off.data_ptr() + o8), vp(mid_len.data_ptr() + o4), PER, BLOCK,
                                                     vp(back.data_ptr()), vp(off.data_ptr() + o8), vp(size.data_ptr() + o4), vp(back_len.data_ptr() + o4), 0)
                assert rc == 0
            torch.cuda.synchronize()

        def stage_set(st):
            sf = seq_first.ctypes.data_as(vp)
            rc = L.crgpu_dict_encode_sequences_dev(g.h, st.h, vp(d_in.data_ptr()), vp(off.data_ptr()), vp(size.data_ptr()), sf, S, BLOCK,
                                                   vp(mid.data_ptr()), vp(mid_off.data_ptr()), vp(mid_len.data_ptr()), 0)
            rc |= L.crgpu_dict_decode_sequences_dev(g.h, st.h, vp(mid.data_ptr()), vp(mid_off.data_ptr()), vp(mid_len.data_ptr()), sf, S, BLOCK,
                                                    vp(back.data_ptr()), vp(off.data_ptr()), vp(size.data_ptr()), vp(back_len.data_ptr()), 0)
            assert rc == 0
            torch.cuda.synchronize()

        def timed(fn, *args):
            torch.cuda.synchronize()
            g.stage_log_read()
            t0 = time.perf_counter()
            r = fn(*args)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            return r, ms, kernel_ms()

        t = {k: [] for k in ("ce", "cs", "cs_k", "se", "se_k", "ss", "ss_k")}
        nodes = 0
        for rep in range(a.reps + 1):                       # repetition 0 warms both paths up and checks them against each other
            for which in ((0, 1) if rep % 2 == 0 else (1, 0)):
                if which == 0:
                    ds, ce, _ = timed(create_each)
                    _, se, se_k = timed(stage_each, ds)
                    each_bytes = (mid_len.clone(), back.clone()) if rep == 0 else None
                    for d in ds:
                        d.close()
                    if rep:
                        t["ce"].append(ce); t["se"].append(se); t["se_k"].append(se_k)
                else:
                    st, cs, cs_k = timed(create_set)
                    _, ss, ss_k = timed(stage_set, st)
                    nodes = sum(st.nodes(i) for i in range(S))
                    if rep == 0:
                        assert torch.equal(mid_len, each_bytes[0]) and torch.equal(back, each_bytes[1]) and torch.equal(back, d_in), "the two paths differ"
                    st.close()
                    if rep:
                        t["cs"].append(cs); t["cs_k"].append(cs_k); t["ss"].append(ss); t["ss_k"].append(ss_k)
        m = {k: statistics.median(v) for k, v in t.items()}
        print(f"{S} | {m['ce']:.2f} | {m['cs']:.2f} ({m['cs_k']:.2f}) | {m['se']:.2f} ({m['se_k']:.2f}) | {m['ss']:.2f} ({m['ss_k']:.2f}) | {nodes}")
    g.close()


if __name__ == "__main__":
    main()
