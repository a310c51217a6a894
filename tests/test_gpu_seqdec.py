"""GPU tests of many sequences of dependent comprop blocks decoded in one launch (crgpu_decode_set,
crgpu_decode_sequences_carried*, crgpu_seqdec.h). The coded blocks come from the ORACLE's encoder run per sequence with
reset=(i == 0), the expected bytes from the oracle's decoder run the same way: every block must come out as the reference's
lzdecode produces it in ITS sequence, whatever the other slots are doing in the same launch."""
import numpy as np
import pytest

import crlib
from comprox_amd import api
from test_gpu_carry import A, B, C, CASES

pytestmark = pytest.mark.gpu

X = crlib.gen_rand(2048, seed=9)
# forty contexts (65 + c, 66) meet 90 different bytes each, so each of their nodes outgrows its line of 62 pairs: the decoder
# counts 20 dense nodes behind block 1 (the cut lies in the middle of context 20) and 40 behind block 2 (read once with
# CrDecodeSet.dense_nodes) — past the CR_V5_DLDS = 32 that live in LDS, which is what the test asserts
DENSE = b"".join(bytes([65 + c, 66, s]) for c in range(40) for s in range(100, 190))
DENSE2 = [DENSE[:(20 * 90 + 45) * 3], DENSE[(20 * 90 + 45) * 3:]]


def _enc(oracle, blocks):
    return [oracle.rop_encode(b, reset=(i == 0)) for i, b in enumerate(blocks)]


def _dec(oracle, coded, caps):
    return [oracle.rop_decode(e, c, reset=(i == 0)) for i, (e, c) in enumerate(zip(coded, caps))]


def test_all_carried_cases_as_sequences_of_one_call(gpu, oracle):
    seqs, coded = [], []
    for _, blocks in CASES:
        e = _enc(oracle, blocks)
        # behind a stored block of 16 bytes or more not even the reference decodes what its encoder wrote (test_gpu_carry.py)
        stored = [i for i, (w, b) in enumerate(zip(e, blocks)) if w[0] == 0 and len(b) >= 16]
        upto = stored[0] + 1 if stored else len(blocks)
        seqs.append([bytes(b) for b in blocks[:upto]])
        coded.append(e[:upto])
    assert [len(s) for s in seqs] == [3, 3, 2, 2, 2, 4, 2, 3]
    caps = [[len(b) for b in s] for s in seqs]
    want = [_dec(oracle, e, c) for e, c in zip(coded, caps)]
    assert want == seqs
    ds = gpu.decode_set_create(len(seqs), 70000)
    try:
        got = gpu.decode_sequences(coded, caps, ds)
    finally:
        ds.close()
    for (name, _), g, w in zip(CASES, got, want):
        assert g == w, f"{name}: blocks {[i for i, (x, y) in enumerate(zip(g, w)) if x != y]} differ"


def test_a_stored_block_leaves_models_and_context_alone(gpu, oracle):
    eA, eB, eC = _enc(oracle, [A, B, C])
    sX = oracle.rop_encode(X)
    assert sX[0] == 0 and len(sX) == 2068
    coded, caps = [eA, sX, eB, eC], [len(A), len(X), len(B), len(C)]
    assert _dec(oracle, coded, caps) == [A, X, B, C]
    ds = gpu.decode_set_create(1, 4096)
    try:
        assert gpu.decode_sequences([coded], [caps], ds) == [[A, X, B, C]]
    finally:
        ds.close()


def test_slices_continue_slots_are_isolated_and_reset_restarts_one(gpu, oracle):
    eA, eB, eC = _enc(oracle, [A, B, C])
    n62 = dict(CASES)["node62"]
    e62 = _enc(oracle, n62)
    n = len(A)
    ds = gpu.decode_set_create(3, 4096)
    try:
        assert gpu.decode_sequences([[eA, eB]] * 3, [[n, n]] * 3, ds) == [[A, B]] * 3
        ds.reset([2])
        assert gpu.decode_sequences([[eC], [], [eA]], [[n], [], [n]], ds) == [[C], [], [A]]
        assert gpu.decode_sequences([[], [eC]], [[], [n]], ds) == [[], [C]]      # slot 1 was not touched by the second call
        ds.reset()
        assert gpu.decode_sequences([[e62[0]]], [[len(n62[0])]], ds) == [[n62[0]]]
        assert gpu.decode_sequences([[e62[1]]], [[len(n62[1])]], ds) == [[n62[1]]]
    finally:
        ds.close()


@pytest.mark.parametrize("calls", [1, 2])
def test_more_dense_nodes_than_lds_holds_across_a_boundary(gpu, oracle, calls):
    coded, caps = _enc(oracle, DENSE2), [len(b) for b in DENSE2]
    assert _dec(oracle, coded, caps) == DENSE2
    ds = gpu.decode_set_create(1, len(DENSE2[0]))
    try:
        if calls == 1:
            got = gpu.decode_sequences([coded], [caps], ds)[0]
        else:                                                   # the second call refills the LDS copies from the arena
            got = gpu.decode_sequences([coded[:1]], [caps[:1]], ds)[0]
            print("dense nodes behind block 1:", ds.dense_nodes(0))
            got += gpu.decode_sequences([coded[1:]], [caps[1:]], ds)[0]
        print("dense nodes behind block 2:", ds.dense_nodes(0))
        assert ds.dense_nodes(0) > 32
    finally:
        ds.close()
    assert got == DENSE2


def test_device_pointer_entry_point_with_gaps(gpu, oracle):
    import torch
    seqs = [[A, B[:15], crlib.gen_text(30000, 45)], [], [X], [C, B]]
    coded = [e for s in seqs for e in _enc(oracle, s)]
    plain = [b for s in seqs for b in s]
    sizes = np.array([len(e) for e in coded], dtype=np.uint32)
    caps = np.array([len(b) for b in plain], dtype=np.uint32)
    in_off = np.cumsum(sizes.astype(np.uint64) + 7) - sizes                 # 7 bytes in front of every coded block
    out_off = np.cumsum(caps.astype(np.uint64) + 13) - caps                 # 13 bytes in front of every output slot
    src = np.zeros(int(in_off[-1]) + int(sizes[-1]) + 1, dtype=np.uint8)
    for o, e in zip(in_off, coded):
        src[int(o):int(o) + len(e)] = np.frombuffer(e, dtype=np.uint8)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()        # noqa: E731
    d_in, d_io, d_sz, d_oo, d_cap = dev(src), dev(in_off.astype(np.uint64)), dev(sizes), dev(out_off.astype(np.uint64)), dev(caps)
    d_out = torch.full((int(out_off[-1]) + int(caps[-1]) + 13,), 0xEE, dtype=torch.uint8, device="cuda")
    d_os = torch.zeros(len(coded) * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ds = gpu.decode_set_create(4, 30000)
    try:
        gpu.decode_sequences_carried_dev(ds, d_in.data_ptr(), d_io.data_ptr(), d_sz.data_ptr(), [0, 3, 3, 4, 6],
                                         d_out.data_ptr(), d_oo.data_ptr(), d_cap.data_ptr(), d_os.data_ptr(), sync=True)
    finally:
        ds.close()
    size, out = d_os.cpu().numpy().view(np.uint32), d_out.cpu().numpy()
    assert [out[int(o):int(o) + int(s)].tobytes() for o, s in zip(out_off, size)] == plain
    for o, c in zip(out_off, caps):                                         # nothing written outside the slots
        assert (out[int(o) - 13:int(o)] == 0xEE).all() and (out[int(o) + int(c):int(o) + int(c) + 13] == 0xEE).all()


def test_a_failure_stays_in_its_sequence_and_poisons_its_slot(gpu, oracle):
    coded, n = _enc(oracle, [A, B, C]), len(A)
    caps = [[n, n, n], [n, n - 1, n], [n, n, n]]                # the header's `total > cap` path: no damaged stream is run
    ds = gpu.decode_set_create(3, 4096)
    try:
        with pytest.raises(Exception, match="-4"):
            gpu.decode_sequences([coded] * 3, caps, ds)
        ds.reset()
        assert gpu.decode_sequences([coded] * 3, caps, ds, strict=False) == [[A, B, C], [A, None, None], [A, B, C]]
        assert gpu.decode_sequences([[], coded[:1]], [[], [n]], ds, strict=False) == [[], [None]]
        ds.reset([1])
        assert gpu.decode_sequences([[], coded], [[], [n, n, n]], ds) == [[], [A, B, C]]
    finally:
        ds.close()


@pytest.mark.parametrize("what", ["rox", "rolz", "too_many_sequences", "descending", "other_context", "oversized_block", "max_block"])
def test_refusals(gpu, oracle, what):
    eA, big = oracle.rop_encode(A), oracle.rop_encode(crlib.gen_rand(5000, seed=3))
    other = api.CrGpu(0) if what == "other_context" else None
    ds = gpu.decode_set_create(2, 4096)
    try:
        with pytest.raises(Exception, match="-2"):
            if what in ("rox", "rolz"):
                gpu.decode_sequences([[eA]], [[len(A)]], ds, codec=api.CODEC_ROX if what == "rox" else api.CODEC_ROLZ)
            elif what == "too_many_sequences":
                gpu.decode_sequences([[eA]] * 3, [[len(A)]] * 3, ds)
            elif what == "descending":
                gpu._decode_sequences_flat([eA] * 3, [len(A)] * 3, [0, 2, 1], ds)
            elif what == "other_context":
                other.decode_sequences([[eA]], [[len(A)]], ds)
            elif what == "oversized_block":
                assert len(big) == 5020 > api.bound(api.CODEC_ROP, 4096)
                gpu.decode_sequences([[big]], [[5000]], ds)
            else:
                gpu.decode_set_create(1, (16 << 20) + 2)
        assert gpu.decode_sequences([[eA]], [[len(A)]], ds) == [[A]]             # a refusal leaves the set usable
    finally:
        ds.close()
        if other:
            other.close()
