"""GPU tests of many sequences of dependent comprop blocks coded in lockstep (crgpu_model_set, crgpu_encode_sequences_carried*,
crgpu_seq.h): every block of every sequence must come out byte for byte as the reference's lzencode writes it in ITS sequence
(the oracle with reset=(i == 0), run per sequence), whatever the other slots of the set are doing in the same step."""
import numpy as np
import pytest

import crlib
from comprox_amd import api
from crlib import A, B, C, CASES

pytestmark = pytest.mark.gpu

T = crlib.gen_text
D = T(4096, 46)


def _expect(oracle, blocks):
    return [oracle.rop_encode(b, reset=(i == 0)) for i, b in enumerate(blocks)]


def _check(got, want, names):
    assert [len(g) for g in got] == [len(w) for w in want]
    for name, gs, ws in zip(names, got, want):
        for i, (g, w) in enumerate(zip(gs, ws)):
            assert g == w, f"{name}: block {i} of {len(ws)} differs ({len(g)} bytes, expected {len(w)})"


@pytest.mark.parametrize("tables", [0, 1], ids=["lds", "tables"])
def test_all_carried_cases_as_sequences_of_one_call(gpu, oracle, tables):
    seqs = [blocks for _, blocks in CASES]                      # 2 to 4 blocks each, 0 to 70 000 bytes: every pre-pass family in one step
    want = [_expect(oracle, s) for s in seqs]
    stored = dict(zip([n for n, _ in CASES], zip(want, seqs)))["stored_between"]
    assert any(w[0] == 0 and len(b) >= 16 for w, b in zip(*stored)), "the case is meant to hold a block that ends stored"
    ms = gpu.model_set_create(len(seqs), 70000)
    gpu.set_option(api.OPT_LZP_TABLES, tables)
    try:
        got = gpu.encode_sequences(seqs, ms)
    finally:
        gpu.set_option(api.OPT_LZP_TABLES, 0)
        ms.close()
    _check(got, want, [n for n, _ in CASES])


def test_aborts_in_the_same_step_undo_only_their_own_slot(gpu, oracle):
    X, Y = crlib.gen_rand(2048, seed=9), crlib.gen_rand(2048, seed=10)
    seqs = [[A, X, B], [A, B, C], [B, Y, A]]
    seqs += [[A, blk, B] for blk in crlib.gen_stored_boundary(oracle.rop_encode, sizes=((1200, 1),), around=1)]
    want = [_expect(oracle, s) for s in seqs]
    assert want[0][1][0] == 0 and want[2][1][0] == 0 and want[1][1][0] != 0     # two abort at step 1, the third codes on
    ms = gpu.model_set_create(len(seqs), 4096)
    try:
        got = gpu.encode_sequences(seqs, ms)
    finally:
        ms.close()
    _check(got, want, ["seq%d" % i for i in range(len(seqs))])


def test_slots_are_isolated_and_keep_their_order(gpu, oracle):
    s3 = [T(5000, 52), T(3000, 53), T(4000, 54)]
    seqs = [[A, B, C], [T(3000, 51), T(2000, 55)], [], s3[:2], [B[:15]], [A, B, C], [T(6000, 56)], []]
    want = [_expect(oracle, s) for s in seqs]
    ms = gpu.model_set_create(8, 6000)
    try:
        got = gpu.encode_sequences(seqs, ms)
        _check(got, want, ["slot%d" % i for i in range(8)])
        assert got[0] == got[5]
        # only slot 3 is fed: it continues its models, every other slot stays as it was
        assert gpu.encode_sequences([[], [], [], s3[2:]], ms)[3] == _expect(oracle, s3)[2:]
        assert gpu.encode_sequences([[D]], ms)[0] == _expect(oracle, [A, B, C, D])[3:]
    finally:
        ms.close()


def test_slices_continue_and_reset_restarts_one_slot(gpu, oracle):
    want4 = _expect(oracle, [A, B, C, D])
    ms = gpu.model_set_create(3, 4096)
    try:
        first = gpu.encode_sequences([[A, B, C, D], [A, B], [A, B]], ms)
        ms.reset([2])
        second = gpu.encode_sequences([[], [C, D], [C, D]], ms)
    finally:
        ms.close()
    assert first[0] == want4 and first[1] + second[1] == want4
    assert first[2] == want4[:2] and second[2] == _expect(oracle, [C, D])


def test_device_pointer_entry_point_with_gaps(gpu, oracle):
    import torch
    seqs = [[A, B[:15], T(30000, 45)], [crlib.gen_rand(2048, seed=9)], [C, B]]
    blocks = [b for s in seqs for b in s]
    sizes = np.array([len(b) for b in blocks], dtype=np.uint32)
    in_off = np.cumsum(sizes.astype(np.uint64) + 7) - sizes                 # 7 bytes in front of every block
    out_off = np.cumsum(sizes.astype(np.uint64) + 33) - sizes - 20          # 13 bytes between the output slots
    src = np.zeros(int(in_off[-1]) + int(sizes[-1]) + 1, dtype=np.uint8)
    for o, b in zip(in_off, blocks):
        src[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()        # noqa: E731
    d_in, d_io, d_sz, d_oo = dev(src), dev(in_off.astype(np.uint64)), dev(sizes), dev(out_off.astype(np.uint64))
    d_out = torch.zeros(int(out_off[-1]) + int(sizes[-1]) + 20, dtype=torch.uint8, device="cuda")
    d_os = torch.zeros(len(blocks) * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = gpu.model_set_create(3, 30000)
    try:
        gpu.encode_sequences_carried_dev(ms, d_in.data_ptr(), d_io.data_ptr(), d_sz.data_ptr(), [0, 3, 4, 6],
                                         d_out.data_ptr(), d_oo.data_ptr(), d_os.data_ptr())
    finally:
        ms.close()
    size, out = d_os.cpu().numpy().view(np.uint32), d_out.cpu().numpy()
    got = [out[int(o):int(o) + int(s)].tobytes() for o, s in zip(out_off, size)]
    assert got == [e for s in seqs for e in _expect(oracle, s)]


def test_refusals(gpu):
    ms = gpu.model_set_create(2, 4096)
    try:
        for codec in (api.CODEC_ROX, api.CODEC_ROLZ):
            with pytest.raises(Exception, match="-2"):
                gpu.encode_sequences([[A]], ms, codec=codec)
        with pytest.raises(Exception, match="-2"):
            gpu.encode_sequences([[A], [A + b"x"]], ms)                      # max_block + 1 bytes
        with pytest.raises(Exception, match="-2"):
            gpu._encode_sequences_flat([A, B, C], [0, 2, 1], ms)             # a descending seq_first
    finally:
        ms.close()
