"""Many sequences of dependent comprop blocks: one crgpu_encode_sequences_carried_dev call (block t of every sequence in one
pass of the pipeline, crgpu_seq.h) against crgpu_encode_blocks_carried_dev called once per sequence, in the same process.

  python tools/seq_rate.py [--runs 5] [--codec rop|rox|rolz] [--out profiles/r10a_seq_rate.txt]

S sequences of 16 blocks of 64 KiB of corpus.enwik_like text with distinct seeds, S = 1, 16, 128, everything in device memory.
Wall clock around the call(s) — both entry points return when the blocks are coded —, the median of --runs after one
warm-up, the two ways alternating; the models are reset in front of every run (inside the clock: a user resets them too) and
the bytes of the two ways must be equal. Then the new call's kernels by name from the stage log, for every S.

--codec rox / rolz (crgpu_seq_lz.h): the path the call replaces is the lzencode shim with carried models — reset_models() and one
lzencode per block on the one-wave coder —, which codes ONE sequence at a time: it is timed on sequence 0 alone, its bytes must
equal the call's for that sequence, and its rate stands for any S. The blocks that came out stored are counted: the abort path
ran once for each.
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


_texts = {}


def sequence_text(s):
    if s not in _texts:
        _texts[s] = corpus.enwik_like(BLOCK * PER_SEQ, seed=100 + s)
    return _texts[s]


class Job:
    """S sequences on the device: the flat block arrays of both entry points"""

    def __init__(self, nseq, codec=api.CODEC_ROP):
        self.nseq, nb, self.codec = nseq, nseq * PER_SEQ, codec
        text = np.concatenate([sequence_text(s) for s in range(nseq)])
        dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()        # noqa: E731
        self.cap = api.bound(codec, BLOCK)
        self.keep = [dev(np.append(text, np.uint8(0))), dev(np.arange(nb, dtype=np.uint64) * BLOCK), dev(np.full(nb, BLOCK, dtype=np.uint32)),
                     dev(np.arange(nb, dtype=np.uint64) * self.cap)]
        self.out = torch.zeros(nb * self.cap, dtype=torch.uint8, device="cuda")
        self.osz = torch.zeros(nb * 4, dtype=torch.uint8, device="cuda")
        self.d_in, self.d_io, self.d_sz, self.d_oo = (t.data_ptr() for t in self.keep)
        self.seq_first = np.arange(nseq + 1, dtype=np.uint32) * PER_SEQ
        self.bytes = nb * BLOCK

    def coded(self):
        size, out = self.osz.cpu().numpy().view(np.uint32), self.out.cpu().numpy()
        return [out[i * self.cap:i * self.cap + int(s)].tobytes() for i, s in enumerate(size)]

    def lockstep(self, gpu, ms):
        self.osz.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms.reset()
        gpu.encode_sequences_carried_dev(ms, self.d_in, self.d_io, self.d_sz, self.seq_first, self.out.data_ptr(), self.d_oo, self.osz.data_ptr(),
                                         codec=self.codec)
        return time.perf_counter() - t0

    def one_by_one(self, gpu, models):
        self.osz.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(self.nseq):
            b = s * PER_SEQ
            models.reset()
            gpu.encode_blocks_carried_dev(models, self.d_in, self.d_io + 8 * b, self.d_sz + 4 * b, PER_SEQ,
                                          self.out.data_ptr(), self.d_oo + 8 * b, self.osz.data_ptr() + 4 * b)
        return time.perf_counter() - t0


def shim_sequence(lib, codec, blocks):
    """reset_models() + one lzencode per block on the library's model-carrying shim: (seconds, coded blocks)"""
    lib.crgpu_shim_config(codec, 0)
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


def main_lz(args, codec):
    lib = comprox_amd.load_library()
    blocks0 = [sequence_text(0)[i * BLOCK:(i + 1) * BLOCK].tobytes() for i in range(PER_SEQ)]
    shim = [shim_sequence(lib, codec, blocks0) for _ in range(args.runs + 1)][1:]
    shim_t, one = statistics.median(t for t, _ in shim), PER_SEQ * BLOCK
    lines = [f"lzencode shim, carried models, reset_models() + {PER_SEQ} calls, one sequence: {shim_t * 1e3:9.1f} ms median of {args.runs} "
             f"(min {min(t for t, _ in shim) * 1e3:.1f}, max {max(t for t, _ in shim) * 1e3:.1f}) = {one / shim_t / 1e6:8.2f} MB/s"]
    gpu, step = comprox_amd.CrGpu(0), {}
    for nseq in SEQS:
        job, ms = Job(nseq, codec), gpu.model_set_create(nseq, BLOCK, codec)
        job.lockstep(gpu, ms)
        coded = job.coded()
        assert coded[:PER_SEQ] == shim[0][1], "the call and the shim wrote different bytes for sequence 0"
        stored = sum(1 for e in coded if e[0 if codec == api.CODEC_ROX else 1] == 0)
        t = [job.lockstep(gpu, ms) for _ in range(args.runs)]
        med = statistics.median(t)
        step[nseq] = med * 1e3 / PER_SEQ
        lines.append(f"S = {nseq:3d} x {PER_SEQ} blocks of 64 KiB: crgpu_encode_sequences_carried_dev, one call {med * 1e3:9.1f} ms median of {args.runs} "
                     f"(min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f}) = {job.bytes / med / 1e6:8.2f} MB/s, {step[nseq]:6.2f} ms per step, "
                     f"{job.bytes / med / (one / shim_t):.1f}x the shim's rate; {sum(map(len, coded))} coded bytes, sequence 0 equal to the shim's, "
                     f"{stored} of {len(coded)} blocks stored (abort path runs)")
        gpu.stage_log(True)
        job.lockstep(gpu, ms)
        for k, (msec, cnt) in sorted(gpu.stage_log_read().items(), key=lambda kv: -kv[1][0]):
            lines.append(f"    {k:20s} {msec:9.2f} ms in {cnt} launches")
        gpu.stage_log(False)
        ms.close()
    lines.append("step time: " + ", ".join(f"S = {k}: {v:.2f} ms" for k, v in step.items()))
    gpu.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--codec", choices=("rop", "rox", "rolz"), default="rop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.codec != "rop":
        text = "\n".join(main_lz(args, api.CODEC_ROX if args.codec == "rox" else api.CODEC_ROLZ))
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    gpu = comprox_amd.CrGpu(0)
    models = gpu.models_create()
    lines, rate = [], {}
    for nseq in SEQS:
        job, ms = Job(nseq), gpu.model_set_create(nseq, BLOCK)
        job.lockstep(gpu, ms)                                                    # warm-up, and the bytes to compare
        new_bytes = job.coded()
        job.one_by_one(gpu, models)
        assert job.coded() == new_bytes, "the two entry points wrote different bytes"
        t = {"new": [], "old": []}
        for _ in range(args.runs):
            t["new"].append(job.lockstep(gpu, ms))
            t["old"].append(job.one_by_one(gpu, models))
        for key, label in (("old", "crgpu_encode_blocks_carried_dev per sequence"), ("new", "crgpu_encode_sequences_carried_dev, one call")):
            med = statistics.median(t[key])
            rate[nseq, key] = (job.bytes / med / 1e6, job.bytes / max(t[key]) / 1e6, job.bytes / min(t[key]) / 1e6)
            lines.append(f"S = {nseq:3d} x {PER_SEQ} blocks of 64 KiB: {label:46s} {med * 1e3:9.1f} ms median of {args.runs} "
                         f"(min {min(t[key]) * 1e3:.1f}, max {max(t[key]) * 1e3:.1f}) = {rate[nseq, key][0]:8.2f} MB/s, {med * 1e3 / PER_SEQ:6.2f} ms per step")
        lines.append(f"S = {nseq:3d}: ratio {statistics.median(t['old']) / statistics.median(t['new']):.2f}x, {sum(map(len, new_bytes))} coded bytes, equal both ways")
        gpu.stage_log(True)
        job.lockstep(gpu, ms)
        for k, (msec, cnt) in sorted(gpu.stage_log_read().items(), key=lambda kv: -kv[1][0]):
            lines.append(f"    {k:20s} {msec:9.2f} ms in {cnt} launches")
        gpu.stage_log(False)
        ms.close()
    lo, hi = SEQS[0], SEQS[-1]
    (m1, a1, b1), (m2, a2, b2) = rate[lo, "new"], rate[hi, "new"]
    verdict = "above" if a2 > b1 else "NOT above"
    lines.append(f"aggregate rate of the new call: S = {lo}: {m1:.2f} MB/s (runs {a1:.2f} .. {b1:.2f}); S = {hi}: {m2:.2f} MB/s (runs {a2:.2f} .. {b2:.2f}): "
                 f"{verdict} the S = {lo} rate by more than the spread of the runs")
    models.close()
    gpu.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
