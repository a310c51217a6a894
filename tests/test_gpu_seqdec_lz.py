"""Many sequences of dependent comprox / comprolz blocks decoded in one launch (k_seqdec_rox_v5 / k_seqdec_rolz_v5). Coded blocks
and expected bytes come from the ORACLE run per sequence with reset=(i == 0) (test_oracle_carried_lz.py anchors it), never from
the GPU. Every block named is coded and does not decode from fresh models: a kernel that drops carried state fails."""
import contextlib

import pytest

import crlib
from comprox_amd import api
from crlib import A, B, C, CASES

pytestmark = pytest.mark.gpu

X = crlib.gen_rand(2048, seed=9)
DENSE = b"".join(bytes([65 + c, 66, s]) for c in range(40) for s in range(100, 190))      # test_gpu_seqdec.py's material
DENSE2 = [DENSE[:(20 * 90 + 45) * 3], DENSE[(20 * 90 + 45) * 3:]]


class Lz:
    def __init__(self, gpu, oracle, which):
        self.gpu, self.which, self.codec = gpu, which, api.CODEC_ROX if which == "rox" else api.CODEC_ROLZ
        self.enc1, self.dec1 = (oracle.rox_encode, oracle.rox_decode) if which == "rox" else (oracle.rolz_encode, oracle.rolz_decode)

    def enc(self, blocks):                  # one sequence; every block must come out coded and decode in its sequence
        coded = [self.enc1(b, reset=(i == 0)) for i, b in enumerate(blocks)]
        assert all(e[0 if self.which == "rox" else 1] != 0 for e in coded)
        assert [self.dec1(e, len(b), reset=(i == 0)) for i, (e, b) in enumerate(zip(coded, blocks))] == blocks
        return coded

    @contextlib.contextmanager
    def decode_set(self, nseq, max_block, grid=0):
        ds = self.gpu.decode_set_create(nseq, max_block, self.codec)
        self.gpu.set_option(api.OPT_SEQDEC_GRID, grid)
        try:
            yield ds, lambda seqs, caps, strict=True, codec=self.codec: self.gpu.decode_sequences(seqs, caps, ds, strict=strict, codec=codec)
        finally:
            self.gpu.set_option(api.OPT_SEQDEC_GRID, 0)
            ds.close()


@pytest.fixture(params=["rox", "rolz"])
def lz(request, gpu, oracle):
    return Lz(gpu, oracle, request.param)


def test_carried_cases_as_sequences_of_one_call(lz):
    seqs = [[bytes(b) for b in dict(CASES)[name]] for name in ("text3", "repeat", "o2_halving", "o1_255", "families")]
    with lz.decode_set(len(seqs), 70000) as (_, decode):
        assert decode([lz.enc(s) for s in seqs], [[len(b) for b in s] for s in seqs]) == seqs


def test_a_stored_block_leaves_models_and_context_alone(lz):
    (eA, eB, eC), sX = lz.enc([A, B, C]), lz.enc1(X)
    assert sX[0 if lz.which == "rox" else 1] == 0 and len(sX) == (2080 if lz.which == "rox" else 2064)
    assert [lz.dec1(e, 4096, reset=(i == 0)) for i, e in enumerate([eA, sX, eB, eC])] == [A, X, B, C]
    with lz.decode_set(1, 4096) as (_, decode):
        assert decode([[eA, sX, eB, eC]], [[len(A), len(X), len(B), len(C)]]) == [[A, X, B, C]]


def test_slices_continue_slots_are_isolated_and_reset_restarts_one(lz):
    (eA, eB, eC), n = lz.enc([A, B, C]), len(A)
    with lz.decode_set(3, 4096) as (ds, decode):
        assert decode([[eA, eB]] * 3, [[n, n]] * 3) == [[A, B]] * 3
        ds.reset([2])
        assert decode([[eC], [], [eA]], [[n], [], [n]]) == [[C], [], [A]]
        assert decode([[], [eC]], [[], [n]]) == [[], [C]]                   # slot 1 was not touched by the second call


@pytest.mark.parametrize("grid", [0, 1])
def test_one_wave_takes_several_sequences(lz, grid):
    """grid = 1: ONE wave walks call 2 in ticket order (most coded bytes first, asserted): slot 0 continues call 1, slot 1 is
    fresh, slot 2's second block fails at the header's `total > cap` (no damaged stream is run), slot 3 continues behind it."""
    plain = [[A, B, C], [A[:3000], B[:3000]], [A[:1200], B[:1200], C[:1200]], [A[:1000], B[:800]]]
    coded, cut = [lz.enc(s) for s in plain], [1, 0, 0, 1]                   # cut: blocks of call 1 per slot
    calls = [[e[:i] for e, i in zip(coded, cut)], [e[i:] for e, i in zip(coded, cut)]]
    caps = [[[len(b) for b in s[:i]] for s, i in zip(plain, cut)], [[len(b) for b in s[i:]] for s, i in zip(plain, cut)]]
    sums = [sum(map(len, seq)) for seq in calls[1]]
    assert all(p > q for p, q in zip(sums, sums[1:])), "no ties, descending: the ticket order is 0, 1, 2, 3"
    caps[1][2][1] -= 1                                                      # slot 2, second block: one byte too little room
    with lz.decode_set(4, 4096, grid) as (_, decode):
        assert decode(calls[0], caps[0]) == [[A], [], [], [A[:1000]]]
        assert decode(calls[1], caps[1], strict=False) == [[B, C], plain[1], [A[:1200], None, None], [B[:800]]]


@pytest.mark.parametrize("ncalls", [1, 2])
def test_more_dense_nodes_than_lds_holds_across_a_boundary(lz, ncalls):
    coded, caps = lz.enc(DENSE2), [len(b) for b in DENSE2]
    with lz.decode_set(1, len(DENSE2[0])) as (ds, decode):
        if ncalls == 1:
            got = decode([coded], [caps])[0]
        else:                                                               # the second call refills the LDS copies from the arena
            got = decode([coded[:1]], [caps[:1]])[0] + decode([coded[1:]], [caps[1:]])[0]
        assert ds.dense_nodes(0) > 32 and got == DENSE2


@pytest.mark.parametrize("what", ["rop", "other_lz", "codec_0", "oversized_block"])
def test_refusals(lz, what):
    eA, big = lz.enc([A])[0], lz.enc1(crlib.gen_rand(10000, seed=3))
    with lz.decode_set(2, 4096) as (_, decode):
        with pytest.raises(Exception, match="-2"):
            if what in ("rop", "other_lz"):
                decode([[eA]], [[len(A)]], codec=api.CODEC_ROP if what == "rop" else api.CODEC_ROX + api.CODEC_ROLZ - lz.codec)
            elif what == "codec_0":
                lz.gpu.decode_set_create(1, 4096, 0)
            else:
                assert len(big) > api.bound(lz.codec, 4096)
                decode([[big]], [[10000]])
        assert decode([[eA]], [[len(A)]]) == [[A]]                          # a refusal leaves the set usable
