"""Many sequences of dependent comprop blocks: one crgpu_encode_sequences_carried_dev call (block t of every sequence in one
pass of the pipeline, crgpu_seq.h) against crgpu_encode_blocks_carried_dev called once per sequence, in the same process.

  python tools/seq_rate.py [--runs 5] [--out profiles/r10a_seq_rate.txt]

S sequences of 16 blocks of 64 KiB of corpus.enwik_like text with distinct seeds, S = 1, 16, 128, everything in device memory.
Wall clock around the call(s) — both entry points return when the blocks are coded —, the median of --runs after one
warm-up, the two ways alternating; the models are reset in front of every run (inside the clock: a user resets them too) and
the bytes of the two ways must be equal. Then the new call's kernels by name from the stage log, for every S.
"""
import argparse
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

    def __init__(self, nseq):
        self.nseq, nb = nseq, nseq * PER_SEQ
        text = np.concatenate([sequence_text(s) for s in range(nseq)])
        dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()        # noqa: E731
        self.cap = api.bound(api.CODEC_ROP, BLOCK)
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
        gpu.encode_sequences_carried_dev(ms, self.d_in, self.d_io, self.d_sz, self.seq_first, self.out.data_ptr(), self.d_oo, self.osz.data_ptr())
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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
