"""Dependent comprop blocks through the reference-signature shim: the one-wave model-carrying coder (with the replay of the
first block that the fast context coded) against the kernel pipeline on carried models (crgpu_shim_pipeline_carry).

  python tools/carry_rate.py [--runs 3] [--out profiles/r09a_carry_rate.txt]

Two sequences of seeded text, each coded by reset_models() + one lzencode per block, wall clock around the whole sequence,
the median of --runs after one warm-up, both ways in the same process; the bytes of the two ways must be equal:
  (a) 33 MiB in three dependent blocks (16 MiB, 16 MiB, the rest) — the case of profiles/r03a_stock_rate.txt;
  (b) 4 MiB in 64 dependent blocks of 64 KiB.
Then the carried pipeline's kernels by name for each sequence (crgpu_encode_blocks_carried with the stage log on).
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch                            # noqa: F401  (first: a process holds one HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import comprox_amd                      # noqa: E402
import crlib                            # noqa: E402
from comprox_amd import api             # noqa: E402


def shim_sequence(lib, blocks, carry: bool):
    lib.crgpu_shim_config(api.CODEC_ROP, 0)
    lib.crgpu_shim_pipeline_carry(1 if carry else 0)
    lib.crgpu_shim_expect_dependent_blocks(0)
    ibs = []
    for b in blocks:
        ib = api.DataBlock()
        lib.data_block_resize(ctypes.byref(ib), len(b))
        ctypes.memmove(ib.m_data, b, len(b))
        ibs.append(ib)
    t0 = time.perf_counter()
    lib.reset_models()
    outs = []
    for ib in ibs:
        ob = api.DataBlock()
        lib.lzencode(ctypes.byref(ib), ctypes.byref(ob), 0)
        outs.append(ob)
    dt = time.perf_counter() - t0
    data = [ctypes.string_at(ob.m_data, ob.m_size) for ob in outs]
    for d in ibs + outs:
        lib.data_block_destroy(ctypes.byref(d))
    return dt, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = comprox_amd.load_library()
    big = crlib.gen_text(33 * 1048576, seed=8)
    small = crlib.gen_text(4 * 1048576, seed=9)
    cases = [("33 MiB in 3 dependent blocks", crlib.split_blocks(big, 16 << 20)),
             ("4 MiB in 64 dependent blocks of 64 KiB", crlib.split_blocks(small, 65536))]
    lines = []
    for name, blocks in cases:
        total = sum(map(len, blocks))
        res = {}
        for carry in (False, True):
            shim_sequence(lib, blocks, carry)                                       # warm-up
            runs = [shim_sequence(lib, blocks, carry) for _ in range(args.runs)]
            res[carry] = (statistics.median(r[0] for r in runs), min(r[0] for r in runs), max(r[0] for r in runs), runs[-1][1])
        assert res[False][3] == res[True][3], "the two paths wrote different bytes"
        for carry, label in ((False, "one-wave coder + replay"), (True, "kernel pipeline, carried models")):
            med, lo, hi, _ = res[carry]
            lines.append(f"{name}: {label}: {med * 1e3:9.1f} ms median of {args.runs} (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}) = {total / med / 1e6:7.2f} MB/s")
        lines.append(f"{name}: ratio {res[False][0] / res[True][0]:.2f}x, {sum(map(len, res[True][3]))} coded bytes, equal both ways")
        g = comprox_amd.CrGpu(0)
        m = g.models_create()
        g.encode_blocks(blocks, models=m)
        m.reset()
        g.stage_log(True)
        g.encode_blocks(blocks, models=m)
        for k, (ms, cnt) in sorted(g.stage_log_read().items(), key=lambda kv: -kv[1][0]):
            lines.append(f"    {k:20s} {ms:9.2f} ms in {cnt} launches")
        g.stage_log(False)
        m.close()
        g.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
