"""Host dicpick() against crgpu_dicpick_dev on the same resident corpus, in one process.

  python tools/dicpick_rate.py [--bytes 100000000] [--seed 8] [--runs 5]

Prints the host pass's seconds (the stream handed over as a file in memory), the device entry point's wall time per
call (the stream already in HBM; best and median of --runs after one warm-up call), the per-kernel milliseconds of one
call from the stage log, tokens / distinct / purges, and the device memory the census holds.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import comprox_amd                      # noqa: E402
from comprox_amd import api, corpus     # noqa: E402


def host_dicpick(lib, data: np.ndarray):
    libc = ctypes.CDLL(None)
    libc.fmemopen.restype = ctypes.c_void_p
    libc.fmemopen.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]
    libc.fclose.argtypes = [ctypes.c_void_p]
    lib.dicpick.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.dicpick.restype = None
    db = api.DataBlock()
    fp = libc.fmemopen(data.ctypes.data_as(ctypes.c_void_p), data.size, b"rb")
    t0 = time.perf_counter()
    lib.dicpick(fp, ctypes.byref(db))
    dt = time.perf_counter() - t0
    libc.fclose(fp)
    text = ctypes.string_at(db.m_data, db.m_size)
    lib.data_block_destroy(ctypes.byref(db))
    return text, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--seed", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.init()                   # torch's HIP runtime first (one runtime per process)
    g = comprox_amd.CrGpu(0)
    data = np.ascontiguousarray(corpus.enwik_like(a.bytes, seed=a.seed))
    dev = torch.from_numpy(data).to("cuda:0")
    torch.cuda.synchronize()
    want, host_s = host_dicpick(g.lib, data)
    got, info = g.dicpick_dev(dev.data_ptr(), data.size)             # warm-up: allocations, code objects
    walls = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        got, info = g.dicpick_dev(dev.data_ptr(), data.size)
        walls.append(time.perf_counter() - t0)
    g.stage_log(True)
    g.dicpick_dev(dev.data_ptr(), data.size)
    stages = g.stage_log_read()
    g.stage_log(False)
    tokens = info["tokens"]
    slots = max(1024, tokens + tokens // 2)
    print(f"corpus: corpus.enwik_like({a.bytes}, seed={a.seed}), dictionary {len(got)} bytes, equal to the host's: {got == want}")
    print(f"host dicpick: {host_s:.3f} s")
    print(f"crgpu_dicpick_dev: best {min(walls) * 1e3:.2f} ms, median {statistics.median(walls) * 1e3:.2f} ms wall per call "
          f"({host_s / min(walls):.1f} x the host), first kernel to last {info['kernel_ms']:.2f} ms, fell_back {info['fell_back']}")
    print(f"tokens {tokens}, distinct {info['distinct']}, purges {info['purges']}")
    print(f"device memory: {(30 * tokens + 12 * (slots - tokens - tokens // 2) + a.bytes // 8192 * 4) / 1e6:.1f} MB "
          f"({slots} slots; 30 bytes per token = {30 * tokens / max(1, a.bytes):.2f} per input byte)")
    for name, (ms, n) in stages.items():
        print(f"  {name:18s} {ms:8.3f} ms  ({n} launch{'es' if n != 1 else ''})")
    print(f"  {'sum':18s} {sum(ms for ms, _ in stages.values()):8.3f} ms")
    g.close()
    return 0 if got == want and not info["fell_back"] else 1


if __name__ == "__main__":
    sys.exit(main())
