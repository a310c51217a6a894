"""GPU tests of many sequences of dependent comprop blocks decoded in one launch (crgpu_decode_set,
crgpu_decode_sequences_carried*, crgpu_seqdec.h). The coded blocks come from the ORACLE's encoder run per sequence with
reset=(i == 0), the expected bytes from the oracle's decoder run the same way: every block must come out as the reference's
lzdecode produces it in ITS sequence, whatever the other slots are doing in the same launch."""
import numpy as np
import pytest

import crlib
from comprox_amd import api
from crlib import A, B, C, CASES

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


# the same over forty other contexts (65 + c, 67): a second sequence whose dense nodes fill the wave's LDS
DENSEB = b"".join(bytes([65 + c, 67, s]) for c in range(40) for s in range(100, 190))


@pytest.mark.parametrize("cap", [0, 1, 2])
def test_a_wave_that_takes_a_second_sequence(gpu, oracle, cap):
    """k_seqdec_v5 is launched with min(resident, sequences) workgroups, and thousands are resident: without a cap no wave ever
    goes round its ticket loop twice. CRGPU_OPT_SEQDEC_GRID = 1 makes ONE wave walk every sequence of a launch in the order
    of the ticket (most coded bytes first; asserted below), so each pick-up meets the LDS the sequence before it left:
      call 1   slot 0: DENSE2[0] (20 dense nodes), slots 1 and 2: A
      call 2   slot 3, fresh: DENSEB, 40 dense nodes, the LDS copies all its own
               slot 0 continues with DENSE2[1]: not fresh; 20 copies come back from the arena, LDS slots 20 .. 31 still hold
                      slot 3's until this block's own nodes take them, and the counter passes CR_V5_DLDS = 32 in the block
               slot 1 continues with B and a piece of C: not fresh, no dense node of its own, the LDS full of the others'
               slot 4, fresh: text, a block that is stored, text — fresh pick-ups reload nothing
               slot 5, fresh: its second block fails through the header's `total > cap` path (no damaged stream is run);
                      that block and the one behind it are None, and
               slot 2, picked up behind it, continues as if nothing had happened; slot 6 has no block
      call 3   slot 0 with all of DENSE again, then slot 3 with the head of DENSEB: both not fresh with a counter of 40, so the
               copies 0 .. 31 come back over the other's and the nodes 32 .. 39 are met in the arena
    All caps must give the oracle's bytes."""
    a, b, c = A[:1200], B[:1200], C[:1200]
    a2, b2, x = A[:2000], B[:2000], crlib.gen_rand(256, seed=9)
    plain = [DENSE2 + [DENSE], [A, B, C[:3000]], [A, B[:1000]], [DENSEB, DENSEB[:5400]], [a2, x, b2], [a, b, c], []]
    coded = [_enc(oracle, s) for s in plain]
    coded[4] = _enc(oracle, [a2, b2])                           # lzdecode leaves the models alone on a stored block: the text
    coded[4].insert(1, oracle.rop_encode(x))                    # behind it continues the text in front of it
    assert coded[4][1][0] == 0 and len(coded[4][1]) == 276
    assert all(e[0] == 1 for s in (0, 1, 2, 3, 5) for e in coded[s])
    want = [_dec(oracle, e, [len(p) for p in s]) for e, s in zip(coded, plain)]
    assert want == plain
    cut = [(1, 2), (1, 3), (1, 2), (0, 1), (0, 3), (0, 3), (0, 0)]          # blocks of calls 1 and 2 per slot; call 3 has the rest
    calls = [[e[:i] for e, (i, j) in zip(coded, cut)], [e[i:j] for e, (i, j) in zip(coded, cut)], [e[j:] for e, (i, j) in zip(coded, cut)]]
    sums = [[sum(map(len, seq)) for seq in call] for call in calls]
    walk = [sorted((s for s in range(7) if call[s]), key=lambda s: -sums[k][s]) for k, call in enumerate(calls)]
    assert walk[1] == [3, 0, 1, 4, 5, 2] and walk[2] == [0, 3]
    assert all(sums[k][p] > sums[k][q] for k in (1, 2) for p, q in zip(walk[k], walk[k][1:])), "no ties: the order is the sizes'"
    caps = [[[len(p) for p in s[:i]] for s, (i, j) in zip(plain, cut)], [[len(p) for p in s[i:j]] for s, (i, j) in zip(plain, cut)],
            [[len(p) for p in s[j:]] for s, (i, j) in zip(plain, cut)]]
    caps[1][5][1] -= 1                                          # slot 5, second block: one byte too little room
    ds = gpu.decode_set_create(7, len(DENSE))
    gpu.set_option(api.OPT_SEQDEC_GRID, cap)
    try:
        got = [gpu.decode_sequences(calls[0], caps[0], ds)]
        print("dense nodes behind call 1:", [ds.dense_nodes(s) for s in range(7)])
        got.append(gpu.decode_sequences(calls[1], caps[1], ds, strict=False))
        print("dense nodes behind call 2:", [ds.dense_nodes(s) for s in range(7)])
        assert ds.dense_nodes(0) > 32 and ds.dense_nodes(3) > 32
        got.append(gpu.decode_sequences(calls[2], caps[2], ds))
    finally:
        gpu.set_option(api.OPT_SEQDEC_GRID, 0)
        ds.close()
    for s, (i, j) in enumerate(cut):
        w = [want[s][:i], want[s][i:j], want[s][j:]]
        if s == 5:
            w[1] = [a, None, None]
        for k in range(3):
            assert got[k][s] == w[k], f"cap {cap}: call {k + 1}, slot {s}: blocks {[n for n, (p, q) in enumerate(zip(got[k][s], w[k])) if p != q]} differ"


def test_fifteen_resets_of_one_slot(gpu, oracle):
    """A slot's order-3 generation has four bits: cr_v3_reset wipes the slot's 8 MiB table when it wraps, which in a decode
    set happens on one slot's sixteenth reset. Slot 0 decodes [A, B] seventeen times, reset in front of each (the set's
    creation was its first reset); slot 1 decodes A in the first round, B in the ninth and C in the last with no reset
    in between — its generations must not move with its neighbour's. (The node generation has sixteen bits: its wrap would
    take 65 536 resets of one slot and is left out.)"""
    coded, n = _enc(oracle, [A, B, C]), len(A)
    assert _dec(oracle, coded, [n, n, n]) == [A, B, C]
    other = {0: 0, 8: 1, 16: 2}
    got1 = []
    ds = gpu.decode_set_create(2, 4096)
    try:
        for r in range(17):
            ds.reset([0])
            mine = [coded[other[r]]] if r in other else []
            got = gpu.decode_sequences([coded[:2], mine], [[n, n], [n] * len(mine)], ds)
            assert got[0] == [A, B], f"round {r}: slot 0, blocks {[i for i, (p, q) in enumerate(zip(got[0], [A, B])) if p != q]} differ"
            got1 += got[1]
    finally:
        ds.close()
    assert got1 == [A, B, C], f"slot 1: blocks {[i for i, (p, q) in enumerate(zip(got1, [A, B, C])) if p != q]} differ"


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
