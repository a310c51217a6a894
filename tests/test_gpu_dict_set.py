"""GPU tests of the dictionary set (crgpu_dict_set): tries built on the device, one dictionary per sequence of blocks in one
launch per kernel, against the CPU oracle's dictionary stage and today's host-built crgpu_dict, bit-exact."""
import ctypes

import numpy as np
import pytest

import comprox_amd
import crlib
import test_oracle_dict as tod

pytestmark = pytest.mark.gpu


def gen_words(n):
    """n distinct lower-case words of 5 .. 19 letters"""
    return [bytes(97 + (i // 26 ** k) % 26 for k in range(4)) + b"q" + b"x" * (i % 15) for i in range(n)]


SHAPES = {
    "none": [], "one": [b"hello"], "the_them": [b"the", b"them"], "them_the": [b"them", b"the"],
    "dup_first": [b"cat", b"cat", b"dog", b"emu"], "dup_last": [b"cat", b"dog", b"emu", b"emu"], "empty_mid": [b"cat", b"", b"dog"],
    "short_long": [b"a", b"abcdefghijklmnopqrst"], "nonletter": [b"http://www.", b"web"], "end_dot": [b"end", b"end."],
    "w64": gen_words(64), "w65": gen_words(65), "w25000": gen_words(25000),
}


def dic_text(words):
    return b"".join(w + b"\n" for w in words)


def probe(words):
    """blocks of a few hundred bytes that hold every (sampled) word followed by ' ', '.', ',', capitalised and at a sentence
    start, each probe with more than 40 bytes behind it"""
    pad = b" 0123456789 0123456789 0123456789 0123456789 "
    some = [w for w in words[::max(1, len(words) // 40)] + words[-1:] if w] or [b"nothing"]
    parts = [b" " + w + b"  " + w + b". " + w + b", " + w.capitalize() + b" again. " + w.capitalize() + b" " + w + b" " + pad for w in some]
    return [b"Start" + b"".join(parts[i:i + 3]) for i in range(0, len(parts), 3)]


def loaded(oracle, text):
    d = crlib.DictOracle(oracle)
    return d, d.load(text, True)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_trie_shapes(name, gpu, oracle):
    words, text = SHAPES[name], dic_text(SHAPES[name])
    parsed = [w + b" " if w[-1:].isalpha() else w for w in words]
    d, nwords = loaded(oracle, text)
    blocks = probe(words)
    want = [d.encode(b) for b in blocks]
    ds, gd = gpu.dict_set_create([text]), gpu.dict_create(text)
    try:
        assert ds.nodes(0) == 1 + len({w[:k] for w in parsed for k in range(1, len(w) + 1)})
        assert ds.words(0) == nwords
        got = ds.encode_sequences([blocks])[0]
        assert got == want
        assert got == gd.encode_blocks(blocks)
        assert ds.decode_sequences([want], [[len(b) for b in blocks]])[0] == blocks
    finally:
        ds.close()
        gd.close()


def test_too_many_lines(gpu):
    with pytest.raises(comprox_amd.CrGpuError):
        gpu.dict_set_create([dic_text(gen_words(25001))])


@pytest.fixture(scope="module")
def world(oracle):
    """six dictionaries, the blocks of their sequences and what the oracle makes of them with the sequence's own dictionary"""
    sources = [crlib.gen_text(70000, seed) for seed in (3, 5, 9)]
    texts = [crlib.DictOracle(oracle).pick(s) for s in sources] + [dic_text(SHAPES[k]) for k in ("none", "them_the", "w25000")]
    seqs = [[sources[0][:65536]],
            [],
            [sources[2][:41], sources[2][:40], b""],
            crlib.split_blocks(sources[0][:20 * 1500], 1500),          # (the text of another dictionary's source: the mapping shows)
            [b" them the them. The " * 30],
            probe(SHAPES["w25000"])[:3]]
    assert [len(s) for s in seqs] == [1, 0, 3, 20, 1, 3]
    enc = []
    for t, s in zip(texts, seqs):
        d, _ = loaded(oracle, t)
        enc.append([d.encode(b) for b in s])
    return texts, seqs, enc


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5), (5, 3, 0, 2, 1, 4)])
def test_several_dictionaries_one_call(order, world, gpu):
    texts, seqs, enc = (([x[i] for i in order]) for x in world)
    ds = gpu.dict_set_create(texts)
    try:
        assert ds.encode_sequences(seqs) == enc
        assert ds.decode_sequences(enc, [[len(b) for b in s] for s in seqs]) == seqs
    finally:
        ds.close()


def test_golden(gpu, oracle):
    text = crlib.gen_text(*tod.GOLD["source"]["args"])
    cs = tod.cases(text)
    names = sorted(cs)
    ds = gpu.dict_set_create([crlib.DictOracle(oracle).pick(text)])
    try:
        assert ds.words(0) == tod.GOLD["words"]
        for k, e in zip(names, ds.encode_sequences([[cs[k] for k in names]])[0]):
            assert (len(e), crlib.sha(e)) == (tod.GOLD["blocks"][k]["size"], tod.GOLD["blocks"][k]["sha256"]), k
    finally:
        ds.close()


def test_words_only_set_and_refusals(world, gpu):
    texts, seqs, enc = world
    caps = [[len(b) for b in s] for s in seqs]
    ds = gpu.dict_set_create(texts, with_trie=False)
    other = comprox_amd.CrGpu(0)
    try:
        assert [ds.nodes(i) for i in range(len(texts))] == [0] * len(texts)
        assert ds.decode_sequences(enc, caps) == seqs
        bad = [list(e) for e in enc]
        bad[3][7] = b"\x01" * 5                                        # too short for the trailer, and not the raw form
        back = ds.decode_sequences(bad, caps, strict=False)
        assert back[3][7] is None and back[3][:7] + back[3][8:] == seqs[3][:7] + seqs[3][8:] and back[:3] + back[4:] == seqs[:3] + seqs[4:]
        with pytest.raises(comprox_amd.CrGpuError):
            ds.decode_sequences(bad, caps)
        for refused in (lambda: ds.encode_sequences(seqs), lambda: gpu.dict_set_create([]), lambda: ds.words(len(texts)),
                        lambda: ds.nodes(len(texts)), lambda: ds.decode_sequences(enc + [[]], caps + [[]])):
            with pytest.raises(comprox_amd.CrGpuError):
                refused()
        L, one, null = gpu.lib, np.zeros(4, dtype=np.uint64), ctypes.c_void_p()
        p = ctypes.c_void_p(one.ctypes.data)
        for first in ([2, 1], [0, 1, 0]):                               # a descending seq_first
            sf = np.array(first, dtype=np.uint32)
            assert L.crgpu_dict_decode_sequences(gpu.h, ds.h, p, p, p, sf.ctypes.data_as(ctypes.c_void_p), len(first) - 1, p, p, p, p) == -2
        sf = np.zeros(2, dtype=np.uint32).ctypes.data_as(ctypes.c_void_p)
        assert L.crgpu_dict_decode_sequences(other.h, ds.h, p, p, p, sf, 1, p, p, p, p) == -2                   # a set of another context
        assert L.crgpu_dict_decode_sequences_dev(gpu.h, ds.h, null, null, null, sf, 1, (16 << 20) + 2, null, null, null, null, 1) == -2
        assert L.crgpu_dict_decode_sequences_dev(gpu.h, ds.h, null, null, null, sf, 1, (16 << 20) + 1, null, null, null, null, 1) == 0
    finally:
        other.close()
        ds.close()
