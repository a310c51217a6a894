"""GPU tests of many sequences of dependent comprox / comprolz blocks coded in lockstep (crgpu_model_set_create_codec,
crgpu_seq_lz.h): every block of every sequence must come out byte for byte as the reference's lzencode writes it in ITS
sequence — the oracle with reset=(i == 0), run per sequence —, stored and tiny blocks included: the models stay where the
token loop gave the block up, side models too, and no block is too small to move them."""
import numpy as np
import pytest

import crlib
from comprox_amd import api
from crlib import A, B, C, CASES

pytestmark = pytest.mark.gpu

T = crlib.gen_text
D = T(4096, 46)
CODEC = {"rox": api.CODEC_ROX, "rolz": api.CODEC_ROLZ}
FLAG = {"rox": 0, "rolz": 1}                                    # the header byte that is 0 in a stored block
TINY = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33)                     # first-token aborts on both sides of each header size


def _enc(oracle, what):
    return getattr(oracle, what + "_encode")


def _expect(oracle, what, blocks):
    return [_enc(oracle, what)(b, reset=(i == 0)) for i, b in enumerate(blocks)]


def _check(got, want, names):
    assert [len(g) for g in got] == [len(w) for w in want]
    for name, gs, ws in zip(names, got, want):
        for i, (g, w) in enumerate(zip(gs, ws)):
            assert g == w, f"{name}: block {i} of {len(ws)} differs ({len(g)} bytes, expected {len(w)})"


def _run(gpu, what, seqs, max_block):
    ms = gpu.model_set_create(len(seqs), max_block, CODEC[what])
    try:
        return gpu.encode_sequences(seqs, ms, codec=CODEC[what])
    finally:
        ms.close()


@pytest.mark.parametrize("tables", [0, 1], ids=["lds", "tables"])
@pytest.mark.parametrize("what", ["rox", "rolz"])
def test_all_carried_cases_as_sequences_of_one_call(gpu, oracle, what, tables):
    seqs = [blocks for _, blocks in CASES]
    want = [_expect(oracle, what, s) for s in seqs]
    assert dict(zip([n for n, _ in CASES], want))["stored_between"][1][FLAG[what]] == 0
    gpu.set_option(api.OPT_LZP_TABLES, tables)
    try:
        got = _run(gpu, what, seqs, 70000)
    finally:
        gpu.set_option(api.OPT_LZP_TABLES, 0)
    _check(got, want, [n for n, _ in CASES])


@pytest.mark.parametrize("what", ["rox", "rolz"])
def test_aborts_and_tiny_blocks_move_only_their_own_slot(gpu, oracle, what):
    enc, stored = _enc(oracle, what), lambda e: e[FLAG[what]] == 0
    X, Y = crlib.gen_rand(2048, seed=9), crlib.gen_rand(2048, seed=10)
    seqs = [[A, X, B], [A, B, C], [B, Y, A], [A, X, X, B], [X, A, B], [A, B, C]]
    seqs += [[A, B[:n], C] for n in TINY]
    behind_a = lambda blk: (enc(A, reset=True), enc(blk, reset=False))[1]          # noqa: E731
    edge = crlib.gen_stored_boundary(behind_a, is_stored=stored, sizes=((1200, 1),), around=1)
    seqs += [[A, blk, B] for blk in edge]
    want = [_expect(oracle, what, s) for s in seqs]
    assert {stored(w[1]) for w in want[-len(edge):]} == {True, False}
    assert stored(want[0][1]) and stored(want[2][1]) and not stored(want[1][1])
    got = _run(gpu, what, seqs, 4096)
    _check(got, want, ["seq%d" % i for i in range(len(seqs))])
    assert got[1] == got[5]


@pytest.mark.parametrize("what", ["rox", "rolz"])
def test_slices_reset_refusals_and_the_empty_block(gpu, oracle, what):
    want4 = _expect(oracle, what, [A, B, C, D])
    codec = CODEC[what]
    ms = gpu.model_set_create(3, 4096, codec)
    try:
        first = gpu.encode_sequences([[A, B, C, D], [A, B], [A, B]], ms, codec=codec)
        ms.reset([2])
        second = gpu.encode_sequences([[], [C, D], [C, D]], ms, codec=codec)
        for other in set(CODEC.values()) - {codec} | {api.CODEC_ROP}:
            with pytest.raises(Exception, match="-2"):
                gpu.encode_sequences([[A]], ms, codec=other)
        ms.reset()
        empty = gpu.encode_sequences([[A, b"", B]], ms, codec=codec)[0]
    finally:
        ms.close()
    assert first[0] == want4 and first[1] + second[1] == want4
    assert first[2] == want4[:2] and second[2] == _expect(oracle, what, [C, D])
    assert empty[1] == gpu.encode_blocks([b""], codec)[0] and [empty[0], empty[2]] == want4[:2]


@pytest.mark.parametrize("what", ["rox", "rolz"])
def test_there_and_back(gpu, what):
    seqs = [blocks for name, blocks in CASES if name in ("text3", "repeat", "families")]
    coded = _run(gpu, what, seqs, 70000)
    assert all(e[FLAG[what]] != 0 for s in coded for e in s)
    ds = gpu.decode_set_create(len(seqs), 70000, CODEC[what])
    try:
        assert gpu.decode_sequences(coded, [[len(b) for b in s] for s in seqs], ds, codec=CODEC[what]) == seqs
    finally:
        ds.close()


@pytest.mark.parametrize("what", ["rox", "rolz"])
def test_device_pointer_entry_point_with_gaps(gpu, oracle, what):
    import torch
    seqs = [[A, B[:15], T(30000, 45)], [crlib.gen_rand(2048, seed=9)], [C, B]]
    blocks = [b for s in seqs for b in s]
    sizes = np.array([len(b) for b in blocks], dtype=np.uint32)
    caps = np.array([api.bound(CODEC[what], int(x)) for x in sizes], dtype=np.uint64)
    in_off = np.cumsum(sizes.astype(np.uint64) + 7) - sizes                 # 7 bytes in front of every block
    out_off = np.cumsum(caps + 13) - caps                                   # 13 bytes between the output slots
    src = np.zeros(int(in_off[-1]) + int(sizes[-1]) + 1, dtype=np.uint8)
    for o, b in zip(in_off, blocks):
        src[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()        # noqa: E731
    d_in, d_io, d_sz, d_oo = dev(src), dev(in_off.astype(np.uint64)), dev(sizes), dev(out_off.astype(np.uint64))
    d_out = torch.zeros(int(out_off[-1]) + int(caps[-1]) + 13, dtype=torch.uint8, device="cuda")
    d_os = torch.zeros(len(blocks) * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = gpu.model_set_create(3, 30000, CODEC[what])
    try:
        gpu.encode_sequences_carried_dev(ms, d_in.data_ptr(), d_io.data_ptr(), d_sz.data_ptr(), [0, 3, 4, 6],
                                         d_out.data_ptr(), d_oo.data_ptr(), d_os.data_ptr(), codec=CODEC[what])
    finally:
        ms.close()
    size, out = d_os.cpu().numpy().view(np.uint32), d_out.cpu().numpy()
    got = [out[int(o):int(o) + int(s)].tobytes() for o, s in zip(out_off, size)]
    assert got == [e for s in seqs for e in _expect(oracle, what, s)]
