"""GPU tests of the device word census (crgpu_dicpick_dev / crgpu_dicpick, csrc/crgpu_dicpick.h): its dictionary text
against the host dicpick() of the same library on the same bytes (pinned to the reference by test_host_dict.py), byte
for byte, with the device path taken (fell_back == 0)."""
import functools

import numpy as np
import pytest

import comprox_amd
import crlib
import test_host_dict as thd
from comprox_amd import api

pytestmark = pytest.mark.gpu

FULL = 25000 * 13 + 1            # live words at which the reference's map purges (cr-dicpick.c:33)
FILL = b"alpha beta, gamma. "    # 19 bytes, every word often enough to be kept


def pick(gpu, data: bytes):
    import torch
    dev = torch.from_numpy(np.frombuffer(data or b"\0", dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return gpu.dicpick_dev(dev.data_ptr(), len(data))


def check(gpu, data: bytes, want: bytes = None, purges: int = 0):
    got, info = pick(gpu, data)
    assert info["fell_back"] == 0
    assert got == (want if want is not None else thd.product_dicpick(comprox_amd.load_library(), data))
    assert info["purges"] == purges
    return info


def records(first: int, count: int) -> bytes:
    """`count` different five-letter words, one per 8-byte record " wwwww, ": laid out from a multiple of 8, no
    200 000-byte chunk costs a word (offset 0 of a chunk is a blank, its zeroed last byte the blank behind the comma)"""
    i = np.arange(first, first + count, dtype=np.int64)
    rec = np.full((count, 8), ord(" "), dtype=np.uint8)
    for k in range(5):
        rec[:, 1 + k] = ord("a") + (i // 26 ** k) % 26
    rec[:, 6] = ord(",")
    return rec.tobytes()


def often(word: bytes, hits: int) -> bytes:
    return (b" " + word + b", ") * hits


WORD_FORMS = (b"a ab " + b"t" * 20 + b" " + b"u" * 21 + b" Hello heLlo HELLO one,two.three:four;five six!seven\neight"
              b" \xe9nine nine\xe9 9ten ten9 1x2 Ab AB aB end. ") * 7 + b"closedbytheend"

NAMES = ["empty", "one", "two", "no_letters", "random", "word_forms", "cut_5_6", "len_199999", "len_200000", "len_200001",
         "len_400000", "word_cap", "text_450k"]


@functools.lru_cache(maxsize=None)
def plain():
    return {
        "empty": b"", "one": b"a", "two": b"ab", "no_letters": b"12 34, 56. " * 100, "random": crlib.gen_rand(10000),
        "word_forms": WORD_FORMS,
        "cut_5_6": often(b"fivehits", 5) + often(b"sixhits", 6) + often(b"sevenhits", 7),
        "len_199999": (FILL * 22000)[:199_999], "len_200000": (FILL * 22000)[:200_000],
        "len_200001": (FILL * 22000)[:200_001], "len_400000": (FILL * 22000)[:400_000],
        # more than 24 998 kept words, two-letter ones among them: the cap, the name-ordered two-byte range, the short-word drop
        "word_cap": records(0, 30_000) * 6 + records(0, 1_000) +
                    b"".join(often(bytes([97 + a, 97 + b]), 6 + a % 3) for a in range(26) for b in range(26)),
        "text_450k": crlib.gen_text(450_000, seed=41),
    }


@pytest.mark.parametrize("name", NAMES)
def test_equals_host_dicpick(gpu, name):
    check(gpu, plain()[name])


def test_golden_source(gpu):
    text = crlib.gen_text(*thd.GOLD["source"]["args"])
    got, info = pick(gpu, text)
    assert info["fell_back"] == 0 and info["purges"] == 0
    assert (len(got), crlib.sha(got)) == (thd.GOLD["dictionary_size"], thd.GOLD["dictionary_sha256"])


def test_chunk_boundary(gpu):
    """" zebra " laid over the end of the first 200 000-byte chunk at every offset: the word ends in front of, on and
    behind the chunk's zeroed last byte, has that byte as its closing byte, starts at offset 0 and 1 of the next chunk.
    Five more hits elsewhere: it is in the dictionary exactly when the occurrence at the boundary counts."""
    base = bytearray((FILL * 22000)[:400_000])
    base[1000:1000 + 40] = (b" zebra, " * 5)
    for at in range(199_990, 200_004):
        data = bytearray(base)
        data[at:at + 7] = b" zebra "
        check(gpu, bytes(data))
    data = bytearray(base)
    data[199_999:200_007] = b"xzebra. "                      # a letter at offset 0 in front of it: no start at offset 1
    check(gpu, bytes(data))


def test_every_lane_and_seam(gpu):
    """the same text behind 0..70 bytes of padding, long enough to cross the tile seam at 8 192 and the waves' seams
    every 2 048 bytes: starts, ends and closing bytes fall on every lane"""
    text = (b"The quick brown fox, jumps. Over: lazy; dogs and " + b"w" * 20 + b" ox A " + b"v" * 19 + b"! no\n") * 150
    want = thd.product_dicpick(comprox_amd.load_library(), b"#" + text)     # (no chunk ends here: the padding changes nothing)
    for shift in range(71):
        check(gpu, b"#" * (shift + 1) + text, want)


@functools.lru_cache(maxsize=None)
def purge_stream(name: str):
    """(stream, host dictionary, purges, different words). w* have 7 hits and v* 6 when the first purge fires, at the last
    of the single words that bring the map to FULL."""
    head = b"".join(often(b"wwwwwww" + bytes([97 + k]), 7) + often(b"vvvvvvv" + bytes([97 + k]), 6) for k in range(10))
    head += b" " * (-len(head) % 8)
    if name == "none":                  # FULL - 1 different words: the map never fills
        data, purges, words = head + records(0, FULL - 1 - 20), 0, FULL - 1
    elif name == "last_token":          # the FULL-th different word is the stream's last token
        data, purges, words = head + records(0, FULL - 20), 1, FULL
    elif name == "return":              # purged words come back: v* start again from 0, w* go on from 7
        data, purges, words = head + records(0, FULL - 20) + head + records(5, 50) * 7, 1, FULL
    else:                               # "two": w* survive (10 live), the singles and 30 more refill the map: the second purge
        data = head + records(0, FULL - 20) + records(0, FULL - 20) + records(400_000, 30) + often(b"vvvvvvva", 6)   # fires at the 20th of them
        purges, words = 2, FULL + 30
    data += b"\n"
    return data, thd.product_dicpick(comprox_amd.load_library(), data), purges, words


@pytest.mark.parametrize("name", ["none", "last_token", "return", "two"])
def test_purge_replay(gpu, name):
    data, want, purges, words = purge_stream(name)
    assert check(gpu, data, want, purges)["distinct"] == words


def test_epoch_cap_hands_over_to_the_host(gpu):
    data, want, _, _ = purge_stream("two")
    gpu.set_option(api.OPT_DICPICK_EPOCHS, 1)
    try:
        got, info = pick(gpu, data)
    finally:
        gpu.set_option(api.OPT_DICPICK_EPOCHS, 256)
    assert info["fell_back"] == 1 and got == want


def test_host_pointer_twin(gpu):
    for data in (plain()["text_450k"], b""):
        got, info = gpu.dicpick(data)
        assert info["fell_back"] == 0 and got == pick(gpu, data)[0]
