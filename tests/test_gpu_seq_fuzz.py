"""Seeded fuzz of the carried (dependent-block) comprop paths on the GPU: crgpu_encode_blocks_carried on one crgpu_models,
crgpu_encode_sequences_carried on a model set and crgpu_decode_sequences_carried on a decode set, fed with the generated
sequences of crlib.gen_carried_sequences — up to twelve blocks of mixed kinds and ragged sizes per sequence, blocks that end
stored first, last, mid-sequence and back to back, calls cut at arbitrary points with slots reset in between. The expectation
is always the oracle run per sequence with reset=(i == 0); tests/test_oracle.py anchors that mode of the oracle to the
reference library on sequences of the same generator."""
import numpy as np
import pytest

import crlib
from comprox_amd import api

pytestmark = pytest.mark.gpu

SLOTS, MAX_BLOCKS, MAX_BLOCK = 24, 12, 6000


def _enc(oracle, blocks):
    return [oracle.rop_encode(b, reset=(i == 0)) for i, b in enumerate(blocks)]


def _dec(oracle, coded, blocks):
    return [oracle.rop_decode(e, len(b), reset=(i == 0)) for i, (e, b) in enumerate(zip(coded, blocks))]


def _same(got, want, what):
    """got, want: per slot a list of blocks; names the first block that differs"""
    assert len(got) == len(want), what
    for s, (gs, ws) in enumerate(zip(got, want)):
        assert len(gs) == len(ws), f"{what}: slot {s} has {len(gs)} blocks, expected {len(ws)}"
        for i, (g, w) in enumerate(zip(gs, ws)):
            assert g == w, (f"{what}: slot {s}, block {i} of {len(ws)} is the first that differs "
                            f"({None if g is None else len(g)} bytes, expected {len(w)})")


def _plan(seed, seqs, fresh):
    """Three calls: every sequence cut at two random points (empty slices allowed); a seeded third of the slots is reset in
    front of the second call and runs its sequence of `fresh` from there, cut once more. Returns (calls, reset slots)."""
    rng = np.random.default_rng(seed + 7000)
    reset = sorted(int(s) for s in rng.choice(len(seqs), len(seqs) // 3, replace=False))
    calls = [[], [], []]
    for s, seq in enumerate(seqs):
        c1, c2 = sorted(int(c) for c in rng.integers(0, len(seq) + 1, 2))
        parts = [seq[:c1], seq[c1:c2], seq[c2:]]
        if s in reset:
            c = int(rng.integers(0, len(fresh[s]) + 1))
            parts[1:] = [fresh[s][:c], fresh[s][c:]]
        for call, part in zip(calls, parts):
            call.append(part)
    return calls, reset


def _cut_like(calls, per_block, seqs, fresh, reset):
    """`per_block` values of seqs / fresh (same shapes), arranged as _plan arranged the blocks"""
    out = [[], [], []]
    for s in range(len(seqs)):
        n1, n2 = len(calls[0][s]), len(calls[1][s])
        if s in reset:
            parts = [per_block[0][s][:n1], per_block[1][s][:n2], per_block[1][s][n2:]]
        else:
            parts = [per_block[0][s][:n1], per_block[0][s][n1:n1 + n2], per_block[0][s][n1 + n2:]]
        for o, part in zip(out, parts):
            o.append(part)
    return out


@pytest.mark.parametrize("seed", [51, 52])
def test_encode_blocks_on_one_models_object(gpu, oracle, seed):
    seqs = crlib.gen_carried_sequences(seed, 4, MAX_BLOCKS)
    want = [_enc(oracle, s) for s in seqs]
    assert sum(len(s) for s in seqs) >= 12
    models = gpu.models_create()
    try:
        got = []
        for k, blocks in enumerate(seqs):
            if k:
                models.reset()
            got.append(gpu.encode_blocks(blocks, models=models))
    finally:
        models.close()
    _same(got, want, f"seed {seed}")


@pytest.mark.parametrize("tables", [0, 1], ids=["lds", "tables"])
@pytest.mark.parametrize("seed", [61, 62])
def test_encode_sequences_in_one_call_and_in_slices_with_resets(gpu, oracle, seed, tables):
    seqs = crlib.gen_carried_sequences(seed, SLOTS, MAX_BLOCKS)
    fresh = crlib.gen_carried_sequences(seed + 100, SLOTS, MAX_BLOCKS)
    want, want_fresh = [_enc(oracle, s) for s in seqs], [_enc(oracle, s) for s in fresh]
    st = [[e[0] == 0 and len(b) >= 16 for e, b in zip(w, s)] for w, s in zip(want, seqs)]
    assert any(a and b for x in st for a, b in zip(x, x[1:])) and any(x and x[0] for x in st) and any(x and x[-1] for x in st), \
        "the seed is meant to hold stored blocks back to back, first and last"
    calls, reset = _plan(seed, seqs, fresh)
    want_calls = _cut_like(calls, (want, want_fresh), seqs, fresh, reset)
    ms = gpu.model_set_create(SLOTS, MAX_BLOCK)
    gpu.set_option(api.OPT_LZP_TABLES, tables)
    try:
        whole = gpu.encode_sequences(seqs, ms)
        ms.reset()
        sliced = []
        for k, call in enumerate(calls):
            if k == 1:
                ms.reset(reset)
            sliced.append(gpu.encode_sequences(call, ms))
    finally:
        gpu.set_option(api.OPT_LZP_TABLES, 0)
        ms.close()
    _same(whole, want, f"seed {seed}, one call")
    for k in range(3):
        _same(sliced[k], want_calls[k], f"seed {seed}, call {k + 1} of 3")
    for s in range(SLOTS):
        if s not in reset:
            assert sliced[0][s] + sliced[1][s] + sliced[2][s] == whole[s], f"seed {seed}: slot {s} in slices is not slot {s} in one call"


@pytest.mark.parametrize("seed", [71, 72])
def test_decode_sequences_in_one_call_and_in_slices_with_resets(gpu, oracle, seed):
    seqs = crlib.gen_carried_sequences(seed, SLOTS, MAX_BLOCKS, decodable=True)
    fresh = crlib.gen_carried_sequences(seed + 100, SLOTS, MAX_BLOCKS, decodable=True)
    # --- with the oracle alone, before anything goes to the GPU
    coded, coded_fresh = [_enc(oracle, s) for s in seqs], [_enc(oracle, s) for s in fresh]
    for c, s in zip(coded + coded_fresh, seqs + fresh):
        cut = crlib.first_stored(c, s)                      # the cap: the decode check leaves no generated block out
        assert cut is None or cut == len(s) - 1, "decodable sequences hold a stored block of 16 bytes or more in last place only"
        assert _dec(oracle, c, s) == [bytes(b) for b in s]
    assert sum(len(s) >= 4 for s in seqs) >= 20, "at least 20 of the 24 sequences are meant to have four blocks or more"
    # ---
    plain, plain_fresh = [[bytes(b) for b in s] for s in seqs], [[bytes(b) for b in s] for s in fresh]
    calls, reset = _plan(seed, coded, coded_fresh)
    want_calls = _cut_like(calls, (plain, plain_fresh), seqs, fresh, reset)
    caps = [[[len(b) for b in part] for part in call] for call in want_calls]
    ds = gpu.decode_set_create(SLOTS, MAX_BLOCK)
    try:
        whole = gpu.decode_sequences(coded, [[len(b) for b in s] for s in seqs], ds)
        ds.reset()
        sliced = []
        for k, call in enumerate(calls):
            if k == 1:
                ds.reset(reset)
            sliced.append(gpu.decode_sequences(call, caps[k], ds))
    finally:
        ds.close()
    _same(whole, plain, f"seed {seed}, one call")
    for k in range(3):
        _same(sliced[k], want_calls[k], f"seed {seed}, call {k + 1} of 3")


def test_blocks_above_64k_through_both_set_entry_points(gpu, oracle):
    text = crlib.gen_text(320000, seed=47)
    blocks = [text[:150000], text[150000:220000], text[220000:]]
    want = _enc(oracle, blocks)
    assert all(w[0] == 1 for w in want) and _dec(oracle, want, blocks) == blocks
    ms = gpu.model_set_create(1, 150000)
    try:
        got = gpu.encode_sequences([blocks], ms)
    finally:
        ms.close()
    _same(got, [want], "encode_sequences")
    ds = gpu.decode_set_create(1, 150000)
    try:
        back = gpu.decode_sequences([want], [[len(b) for b in blocks]], ds)
    finally:
        ds.close()
    _same(back, [blocks], "decode_sequences")
