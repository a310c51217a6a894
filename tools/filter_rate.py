"""The `-F` filters over a stream that is resident in device memory: the host pass against crgpu_filter_blocks_dev.

  python tools/filter_rate.py [--bytes 100000000] [--block 65536] [--runs 5] [--out profiles/r08a_filter_rate.txt]

The stream is seeded pieces of crlib.gen_text / gen_pe / gen_elf / gen_bmp, about half of it images. Timed, each the
median of --runs after one warm-up, FILTER_ENC from a fresh state:
  (a) filter_inplace block by block over a host copy (the pass alone);
  (b) the same with the copies a resident stream needs for it: device -> pinned host memory, the pass, host -> device;
  (c) crgpu_filter_blocks_dev, wall clock: scan, readbacks, plan, snapshot and kernels, with the kernels' times by name.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import comprox_amd                      # noqa: E402
import crlib                            # noqa: E402


def make_stream(n: int) -> bytes:
    text = crlib.gen_text(n // 2 + 4096, seed=8)
    images = [crlib.gen_pe(300_000, 5), crlib.gen_bmp(640, 480, 24, 7), crlib.gen_elf(200_000, 6), crlib.gen_bmp(500, 300, 32, 9),
              crlib.gen_pe(90_000, 11, nsec=5), crlib.gen_elf(450_000, 12), crlib.gen_bmp(1021, 333, 24, 13)]
    out, size, at, k = [], 0, 0, 0
    while size < n:
        img = images[k % len(images)]
        piece = text[at:at + len(img)]
        at, k = at + len(piece), k + 1
        out += [piece, img]
        size += len(piece) + len(img)
    return b"".join(out)[:n]


def host_pass(lib, buf: np.ndarray, block: int):
    lib.crgpu_filter_reset()
    base = buf.ctypes.data
    return [lib.filter_inplace(ctypes.c_void_p(base + o), min(block, buf.size - o), 0) for o in range(0, buf.size, block)]


def median_of(fn, runs):
    fn()
    times = []
    for _ in range(runs):
        times.append(fn())
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=100_000_000)
    ap.add_argument("--block", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08a_filter_rate.txt"))
    a = ap.parse_args()
    torch.cuda.init()                   # torch's HIP runtime first (one runtime per process)
    g = comprox_amd.CrGpu(0)
    lib = g.lib
    lib.filter_inplace.restype = ctypes.c_int
    lib.filter_inplace.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int]
    data = np.frombuffer(make_stream(a.bytes), dtype=np.uint8)
    n = data.size
    off = list(range(0, n, a.block))
    lens = [min(a.block, n - o) for o in off]
    orig = torch.from_numpy(data.copy()).to("cuda:0")
    dev = torch.empty_like(orig)
    pinned = torch.empty(n, dtype=torch.uint8).pin_memory()
    work = np.empty_like(data)

    def run_a():
        work[:] = data
        t0 = time.perf_counter()
        run_a.rets = host_pass(lib, work, a.block)
        return time.perf_counter() - t0

    def run_b():
        dev.copy_(orig)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(dev)
        torch.cuda.synchronize()
        host_pass(lib, pinned.numpy(), a.block)
        dev.copy_(pinned)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def run_c():
        dev.copy_(orig)
        torch.cuda.synchronize()
        lib.crgpu_filter_reset()
        t0 = time.perf_counter()
        run_c.touched, run_c.info = g.filter_blocks_dev(dev.data_ptr(), off, lens, 0)
        return time.perf_counter() - t0

    t_a, t_b = median_of(run_a, a.runs), median_of(run_b, a.runs)
    same_b = bool((dev.cpu().numpy() == work).all())
    t_c = median_of(run_c, a.runs)
    same_c = bool((dev.cpu().numpy() == work).all()) and run_c.touched == run_a.rets
    g.stage_log(True)
    t_logged = run_c()
    stages = g.stage_log_read()
    g.stage_log(False)
    info = run_c.info
    kernels = sum(ms for ms, _ in stages.values())
    lines = [f"stream: {n} bytes, blocks of {a.block}, {sum(run_a.rets)} of {len(off)} blocks touched; median of {a.runs} after a warm-up",
             f"(a) host filter_inplace alone:             {t_a * 1e3:9.2f} ms  ({n / t_a / 1e6:8.1f} MB/s)",
             f"(b) D2H + host filter_inplace + H2D:       {t_b * 1e3:9.2f} ms  ({n / t_b / 1e6:8.1f} MB/s)  bytes equal to (a): {same_b}",
             f"(c) crgpu_filter_blocks_dev, wall clock:   {t_c * 1e3:9.2f} ms  ({n / t_c / 1e6:8.1f} MB/s)  bytes and returns equal to (a): {same_c}",
             f"    headers {info['images']}, pieces {info['pieces']}, fell_back {info['fell_back']}; kernels of that call {info['kernel_ms']:.3f} ms",
             f"    one more call with the stage log on: {t_logged * 1e3:.2f} ms wall, {kernels:.3f} ms in kernels, "
             f"{t_logged * 1e3 - kernels:.2f} ms in readbacks, plan, uploads and the snapshot copy; its kernels by name:"]
    lines += [f"      {name:18s} {ms:8.3f} ms  ({cnt} launch{'es' if cnt != 1 else ''})" for name, (ms, cnt) in stages.items()]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    g.close()
    return 0 if same_b and same_c and not info["fell_back"] else 1


if __name__ == "__main__":
    sys.exit(main())
