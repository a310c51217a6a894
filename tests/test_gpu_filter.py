"""GPU tests of the device `-F` filters (crgpu_filter_blocks_dev / crgpu_filter_blocks, csrc/crgpu_filter.h): bytes and
return values against filter_inplace of the same library run block by block on a host copy (test_host_filter.run, which
test_host_filter.py pins to the reference), in both directions, with the device path taken unless stated."""
import numpy as np
import pytest

import crlib
import test_host_filter as thf
from test_host_filter import GOLD, lib  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

PE_CODE = 368            # gen_pe: the code range starts 24 + 224 + 3 * 40 bytes into the file (pe_step's quirk)


def layout(n, block):
    off = list(range(0, max(n, 1), block))
    return off, [min(block, n - o) for o in off]


def device(gpu, lib, data, block, mode, reset=True):
    import torch
    if reset:
        lib.crgpu_filter_reset()
    dev = torch.from_numpy(np.frombuffer(data or b"\0", dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    off, lens = layout(len(data), block)
    touched, info = gpu.filter_blocks_dev(dev.data_ptr(), off, lens, mode)
    return touched, dev.cpu().numpy().tobytes()[:len(data)], info


def check(gpu, lib, data, block, fell_back=0):
    """encode, then decode the encoded stream: device == host in bytes, returns, lossy count and fell_back"""
    src = data
    for mode in (0, 1):
        rets, want = thf.run(lib, src, block, mode)
        lossy = lib.crgpu_filter_lossy()
        touched, got, info = device(gpu, lib, src, block, mode)
        assert got == want, next(i for i in range(len(want)) if got[i] != want[i])
        assert touched == rets and lib.crgpu_filter_lossy() == lossy
        assert info["fell_back"] == fell_back
        src = want
        enc = enc if mode else want
    return enc, src


@pytest.mark.parametrize("name", sorted(GOLD["cases"]))
def test_golden_streams(gpu, lib, name):
    g = GOLD["cases"][name]
    enc, dec = check(gpu, lib, thf.build(g["specs"]), g["block"])
    assert crlib.sha(enc) == g["enc_sha256"] and crlib.sha(dec) == g["dec_sha256"]
    assert lib.crgpu_filter_lossy() == {"two_elf": 1, "tar_like": 2}.get(name, 0)


@pytest.mark.parametrize("name", ["two_elf", "tar_like"])
def test_restart_mode(gpu, lib, name):
    g = GOLD["cases"][name]
    data = thf.build(g["specs"])
    assert lib.crgpu_filter_set_mode(1) == 0
    try:
        enc, dec = check(gpu, lib, data, g["block"])
        assert dec == data and crlib.sha(enc) != g["enc_sha256"] and lib.crgpu_filter_lossy() == 0
    finally:
        lib.crgpu_filter_set_mode(0)


@pytest.mark.parametrize("pattern", [b"\xe8", b"\xe8\xe9\x00" + b"\xe8" * 400])
@pytest.mark.parametrize("start", [64 * 3 - 3, 4096 - 3, 16384 - 3, 20000 - PE_CODE - 7])
def test_automaton_seams(gpu, lib, start, pattern):
    """runs of opcodes never synchronise the skip state: they cross byte 63/64 of a lane, a wave's 4 KiB, a tile's 16 KiB
    and the end of the 20 000-byte block; lengths 203 and 137 are no multiples of 5"""
    pe = bytearray(crlib.gen_pe(40000))
    for at, n in ((start, 203), (start + 1000, 137)):
        pe[PE_CODE + at:PE_CODE + at + n] = (pattern * n)[:n]
    check(gpu, lib, bytes(pe), 20000)


def limit_cases():
    tail = crlib.gen_pe(10005 - PE_CODE)                   # the image's last piece: 5 bytes at the start of block 1
    ops = bytearray(crlib.gen_pe(5000))
    ops[PE_CODE + 5000 - 9:PE_CODE + 5000] = b"\xe8" * 9   # an opcode in each of the last 9 bytes of the piece
    elf = bytearray(crlib.gen_elf(30000))
    elf[8990:9000] = b"\xe8" * 10                          # operands that would cross the end of the 9 000-byte block
    return {"short_piece": (tail + crlib.gen_text(300), 10000), "last_nine": (bytes(ops), 1 << 20), "avail": (bytes(elf), 9000),
            "large_piece": (crlib.gen_pe(199000), 200000)}


@pytest.mark.parametrize("name", sorted(limit_cases()))
def test_limits_and_one_large_piece(gpu, lib, name):
    check(gpu, lib, *limit_cases()[name])


def bmp_cases():
    neg = bytearray(crlib.gen_bmp(20, 10))
    neg[22:26] = (-10 & 0xFFFFFFFF).to_bytes(4, "little")
    return {"width4": (crlib.gen_bmp(4, 9), 1 << 20), "padding": (crlib.gen_bmp(37, 11), 1 << 20), "bpp32": (crlib.gen_bmp(33, 12, 32), 1 << 20),
            "negative_height": (bytes(neg), 1 << 20), "rows_cut": (crlib.gen_bmp(100, 40), 1000), "shorter_than_row": (crlib.gen_bmp(100, 12), 250),
            "trailer": (crlib.gen_bmp(16, 16, trailer=b"xyz" * 50) + crlib.gen_text(500), 1 << 20), "long_row": (crlib.gen_bmp(6000, 4), 1 << 20)}


@pytest.mark.parametrize("name", sorted(bmp_cases()))
def test_bmp(gpu, lib, name):
    check(gpu, lib, *bmp_cases()[name])


def test_state_is_shared_with_the_host_pass(gpu, lib):
    g = GOLD["cases"]["mixed"]
    data, block = thf.build(g["specs"]), g["block"]
    rets, want = thf.run(lib, data, block, 0)
    assert len(rets) == 4
    half = 2 * block
    for first, second in (("dev", "dev"), ("dev", "host"), ("host", "dev")):
        lib.crgpu_filter_reset()
        out, got_rets = b"", []
        for how, part in ((first, data[:half]), (second, data[half:])):
            if how == "dev":
                t, b, info = device(gpu, lib, part, block, 0, reset=False)
                assert info["fell_back"] == 0
            else:
                t, b = [], b""
                for i in range(0, len(part), block):
                    buf = bytearray(part[i:i + block])
                    c = (thf.ctypes.c_char * len(buf)).from_buffer(buf)
                    t.append(lib.filter_inplace(c, len(buf), 0))
                    b += bytes(buf)
            out, got_rets = out + b, got_rets + t
        assert out == want and got_rets == rets, (first, second)
    assert device(gpu, lib, data, block, 0)[1] == want           # after crgpu_filter_reset(): the same bytes again


def test_blocks_apart(gpu, lib):
    """blocks with gaps between them (the snapshot holds the blocks packed): nothing between them is read as a header or written"""
    import torch
    g = GOLD["cases"]["mixed"]
    data, block = thf.build(g["specs"]), g["block"]
    rets, want = thf.run(lib, data, block, 0)
    gap = b"MZBM\x7fELF" * 100
    off, lens = layout(len(data), block)
    far = [o + (i + 1) * len(gap) for i, o in enumerate(off)]
    dev = torch.from_numpy(np.frombuffer(b"".join(gap + data[o:o + n] for o, n in zip(off, lens)) + gap, dtype=np.uint8).copy()).to("cuda:0")
    lib.crgpu_filter_reset()
    touched, info = gpu.filter_blocks_dev(dev.data_ptr(), far, lens, 0)
    assert touched == rets and info["fell_back"] == 0
    assert dev.cpu().numpy().tobytes() == b"".join(gap + want[o:o + n] for o, n in zip(off, lens)) + gap


def test_overhang_hands_over_to_the_host(gpu, lib):
    """an ELF image that ends inside its block is converted up to 48 bytes past the 2 948 it claims; a signature there"""
    data = crlib.gen_elf(3000) + crlib.gen_text(2000)
    check(gpu, lib, data, 1 << 20)
    poked = bytearray(data)
    poked[2960:2962] = b"MZ"
    check(gpu, lib, bytes(poked), 1 << 20, fell_back=1)


def test_degenerate(gpu, lib):
    assert gpu.filter_blocks_dev(0, [], [], 0)[0] == []
    for data in (b"", b"M", thf.build(GOLD["cases"]["plain_text"]["specs"])):
        touched, got, info = device(gpu, lib, data, 4096, 0)
        assert got == data and not any(touched) and info["pieces"] == 0 and info["fell_back"] == 0


def test_host_pointer_twin(gpu, lib):
    g = GOLD["cases"]["mixed"]
    data = thf.build(g["specs"])
    rets, want = thf.run(lib, data, g["block"], 0)
    lib.crgpu_filter_reset()
    got, touched, info = gpu.filter_blocks(data, *layout(len(data), g["block"]), 0)
    assert got == want and touched == rets and info["fell_back"] == 0
