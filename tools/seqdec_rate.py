"""Many sequences of dependent comprop (or, --codec, comprox / comprolz) blocks DECODED: one crgpu_decode_sequences_carried_dev call (one wave per sequence, one
launch, crgpu_seqdec.h) against the only other way to decode the same bytes — reset_models() + lzdecode block after block
through the shim, one sequence after the other — in the same process.

  python tools/seqdec_rate.py [--codec rop|rox|rolz] [--runs 5] [--out profiles/r11a_seqdec_rate.txt]

S sequences of 16 blocks of 64 KiB of corpus.enwik_like text with distinct seeds, S = 1, 16, 128, encoded once with
encode_sequences. The new call: everything in device memory, wall clock around reset + the call (sync), the median of --runs
after one warm-up. The shim: ONE sequence (its rate does not depend on how many follow), the same clock and median. Both must
return the original bytes. Expectation on record: the S = 128 aggregate rate is at least 64 x the shim's one-sequence rate.
comprox / comprolz have no carried encoder on the kernel pipeline: their sequences are coded by the lzencode shim with models
carried, 16 distinct ones, and sequence s of a larger S is sequence s % 16 again (on a slot of its own). Also printed: the
S = 128 call time over the S = 1 call time.
Last, what a lone chain costs: the S = 1 time next to one crgpu_decode_blocks_dev call on 16 INDEPENDENT blocks of that size.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch                            # noqa: F401  (first: a process holds one HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import comprox_amd                      # noqa: E402
from comprox_amd import api, corpus     # noqa: E402

BLOCK, PER_SEQ, SEQS = 65536, 16, (1, 16, 128)
CODECS = {"rop": (api.CODEC_ROP, "k_seqdec_v5"), "rox": (api.CODEC_ROX, "k_seqdec_rox_v5"), "rolz": (api.CODEC_ROLZ, "k_seqdec_rolz_v5")}
DISTINCT = 16                           # comprox / comprolz: sequences coded through the shim


def cut(s):
    text = corpus.enwik_like(BLOCK * PER_SEQ, seed=100 + s).tobytes()
    return [text[i:i + BLOCK] for i in range(0, len(text), BLOCK)]


class Job:
    """coded blocks on the device, flat, with room for every decoded block"""

    def __init__(self, coded):
        nb = len(coded)
        sizes = np.array([len(e) for e in coded], dtype=np.uint32)
        in_off = np.concatenate(([0], np.cumsum(sizes[:-1], dtype=np.uint64))).astype(np.uint64)
        dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()        # noqa: E731
        self.keep = [dev(np.frombuffer(b"".join(coded) + b"\0", dtype=np.uint8)), dev(in_off), dev(sizes),
                     dev(np.arange(nb, dtype=np.uint64) * BLOCK), dev(np.full(nb, BLOCK, dtype=np.uint32))]
        self.out = torch.zeros(nb * BLOCK, dtype=torch.uint8, device="cuda")
        self.osz = torch.zeros(nb * 4, dtype=torch.uint8, device="cuda")
        self.d_in, self.d_io, self.d_sz, self.d_oo, self.d_cap = (t.data_ptr() for t in self.keep)
        self.nb, self.bytes = nb, nb * BLOCK

    def clear(self):
        self.out.zero_()
        self.osz.zero_()
        torch.cuda.synchronize()

    def decoded(self):
        assert (self.osz.cpu().numpy().view(np.uint32) == BLOCK).all()
        return self.out.cpu().numpy().tobytes()

    def sequences(self, gpu, ds):
        self.clear()
        t0 = time.perf_counter()
        ds.reset()
        gpu.decode_sequences_carried_dev(ds, self.d_in, self.d_io, self.d_sz, np.arange(self.nb // PER_SEQ + 1, dtype=np.uint32) * PER_SEQ,
                                         self.out.data_ptr(), self.d_oo, self.d_cap, self.osz.data_ptr(), sync=True, codec=ds.codec)
        return time.perf_counter() - t0

    def independent(self, gpu, codec):
        self.clear()
        t0 = time.perf_counter()
        gpu.decode_blocks_dev(codec, self.d_in, self.d_io, self.d_sz, self.nb, BLOCK, self.out.data_ptr(), self.d_oo, self.d_cap,
                              self.osz.data_ptr(), sync=True)
        return time.perf_counter() - t0


def shim_sequence(L, coded, fn=None):
    """reset_models() + lzdecode (or fn = L.lzencode) block after block on the library's model-carrying context; returns
    (seconds, list of blocks)"""
    fn = fn or L.lzdecode
    out = []
    t0 = time.perf_counter()
    L.reset_models()
    for e in coded:
        ib, ob = api.DataBlock(), api.DataBlock()
        L.data_block_resize(ctypes.byref(ib), len(e))
        ctypes.memmove(ib.m_data, e, len(e))
        fn(ctypes.byref(ib), ctypes.byref(ob), 0)
        out.append(ctypes.string_at(ob.m_data, ob.m_size))
        L.data_block_destroy(ctypes.byref(ib))
        L.data_block_destroy(ctypes.byref(ob))
    return time.perf_counter() - t0, out


def med_line(label, times, nbytes, runs):
    med = statistics.median(times)
    return med, (f"{label:62s} {med * 1e3:9.1f} ms median of {runs} (min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f}) "
                 f"= {nbytes / med / 1e6:8.2f} MB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--codec", choices=sorted(CODECS), default="rop")
    args = ap.parse_args()
    codec, kernel = CODECS[args.codec]
    gpu = comprox_amd.CrGpu(0)
    L = api.load_library()
    L.crgpu_shim_config(codec, 0)
    L.crgpu_shim_pipeline_carry(0)
    if codec == api.CODEC_ROP:
        plain = [cut(s) for s in range(SEQS[-1])]
        ms = gpu.model_set_create(SEQS[-1], BLOCK)
        coded = gpu.encode_sequences(plain, ms)
        ms.close()
    else:
        L.crgpu_shim_expect_dependent_blocks(1)
        plain = [cut(s % DISTINCT) for s in range(SEQS[-1])]
        distinct = [shim_sequence(L, plain[s], L.lzencode)[1] for s in range(DISTINCT)]
        coded = [distinct[s % DISTINCT] for s in range(SEQS[-1])]
    lines, rate, call = [], {}, {}

    assert shim_sequence(L, coded[0])[1] == plain[0], "the shim did not return the original bytes"                    # (warm-up)
    shim_med, line = med_line("shim: reset_models() + lzdecode x 16, one sequence", [shim_sequence(L, coded[0])[0] for _ in range(args.runs)],
                              BLOCK * PER_SEQ, args.runs)
    shim_rate = BLOCK * PER_SEQ / shim_med / 1e6
    lines.append(line)

    for nseq in SEQS:
        job, ds = Job([e for s in coded[:nseq] for e in s]), gpu.decode_set_create(nseq, BLOCK, codec)
        job.sequences(gpu, ds)                                                   # warm-up, and the bytes to compare
        assert job.decoded() == b"".join(b for s in plain[:nseq] for b in s), "crgpu_decode_sequences_carried_dev did not return the original bytes"
        times = [job.sequences(gpu, ds) for _ in range(args.runs)]
        med, line = med_line(f"S = {nseq:3d} x {PER_SEQ} blocks of 64 KiB: crgpu_decode_sequences_carried_dev", times, job.bytes, args.runs)
        rate[nseq], call[nseq] = job.bytes / med / 1e6, med
        lines.append(line)
        lines.append(f"    {kernel} {gpu.last_kernel_ms():9.2f} ms (last run); {rate[nseq] / shim_rate:7.2f} x the shim's one-sequence rate; original bytes both ways")
        if nseq == 1:
            ind = gpu.encode_blocks(plain[0], codec)
            jb = Job(ind)
            jb.independent(gpu, codec)
            assert jb.decoded() == b"".join(plain[0])
            lines.append(med_line("    beside it: crgpu_decode_blocks_dev, 16 independent blocks", [jb.independent(gpu, codec) for _ in range(args.runs)], jb.bytes, args.runs)[1])
        ds.close()
    ratio = rate[SEQS[-1]] / shim_rate
    lines.append(f"S = {SEQS[-1]} aggregate {rate[SEQS[-1]]:.2f} MB/s = {ratio:.1f} x the shim's {shim_rate:.2f} MB/s: "
                 f"{'at least' if ratio >= 64 else 'BELOW'} the 64 x expected")
    lines.append(f"S = {SEQS[-1]} call / S = {SEQS[0]} call: {call[SEQS[-1]] * 1e3:.1f} / {call[SEQS[0]] * 1e3:.1f} ms = {call[SEQS[-1]] / call[SEQS[0]]:.2f}")
    gpu.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
