"""The device generator without a GPU: csrc/gs_rand.cuh compiled for the host (tests/twin/host_rand.cpp) against the
Python model (tests/randvec.py) and single blocks from OpenSSL (tests/golden/chacha20_blocks.json), and the boundary
checks of the new entry points (declared, exported, listed)."""
import ctypes
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import randvec as rv
from gsutil import HERE, REPO, curve

CURVES = ["bls12_381", "bn254"]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
TWIN_SRC = os.path.join(HERE, "twin", "host_rand.cpp")
RAND_HDR = os.path.join(REPO, "groth_sahai_rs_amd", "csrc", "gs_rand.cuh")

NAMES = ["gs_rand_set_key", "gs_rand_fr_dev", "gs_rand_fr", "gs_rand_rho_dev", "gs_rand_rho",
         "gs_prove_batch_drawn_dev", "gs_prove_batch_drawn", "gs_prove_statement_drawn_dev", "gs_prove_statement_drawn",
         "gs_rerandomize_batch_drawn_dev", "gs_rerandomize_batch_drawn", "gs_rerandomize_statement_drawn_dev",
         "gs_rerandomize_statement_drawn"]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    # a missing source or compiler FAILS: nothing here may pass by skipping
    assert os.path.exists(TWIN_SRC), "missing " + TWIN_SRC
    assert os.path.exists(RAND_HDR), "missing " + RAND_HDR
    assert os.path.exists(CLANG), "no host clang++ for the CPU twin: " + CLANG
    so = str(tmp_path_factory.mktemp("rand_twin") / "libhost_rand.so")
    subprocess.check_call([CLANG, "-O2", "-std=c++17", "-Wno-psabi", "-shared", "-fPIC", TWIN_SRC, "-o", so])
    lib = ctypes.CDLL(so)
    lib.twin_chacha20_block.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p]
    lib.twin_rand_block.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p]
    for c in CURVES:
        getattr(lib, "twin_block_to_fr_" + c).argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    lib.twin_block_rho.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(HERE, "golden", "chacha20_blocks.json")) as f:
        return json.load(f)["cases"]


def twin_block(twin, key, counter, nonce):
    out = ctypes.create_string_buffer(64)
    twin.twin_chacha20_block(key, counter, nonce, out)
    return out.raw


def twin_fr(twin, cname, blk):
    out = np.zeros(4, dtype=np.uint64)
    getattr(twin, "twin_block_to_fr_" + cname)(blk, out.ctypes.data)
    return out


def twin_rho(twin, blk):
    out = np.zeros(8, dtype=np.uint64)
    twin.twin_block_rho(blk, out.ctypes.data)
    return [int(x) for x in out]


def test_fixture_covers_the_named_cases(fixture):
    names = {c["name"] for c in fixture}
    assert "rfc8439_2_3_2" in names
    assert any(c["counter"] == 0 for c in fixture) and any(c["counter"] == 0xFFFFFFFF for c in fixture)
    assert any(c["key"] == "00" * 32 for c in fixture) and any(c["key"] == "ff" * 32 for c in fixture)
    assert any(all(b != 0 for b in bytes.fromhex(c["nonce"])) for c in fixture)
    assert all(len(c["block"]) == 128 for c in fixture)  # ONE block each: nothing crosses 2^32


def test_block_twin_model_fixture(twin, fixture):
    for c in fixture:
        key, nonce, want = bytes.fromhex(c["key"]), bytes.fromhex(c["nonce"]), bytes.fromhex(c["block"])
        assert rv.chacha20_block(key, c["counter"], nonce) == want, "model: " + c["name"]
        assert twin_block(twin, key, c["counter"], nonce) == want, "twin: " + c["name"]


def test_rfc_block_in_this_interface(twin):
    """RFC 8439 section 2.3.2 is domain 0x09000000, stream 0x4a000000, first 1."""
    want = bytes.fromhex(rv.RFC_BLOCK_HEX)
    assert rv.nonce_of(rv.RFC_DOMAIN, rv.RFC_STREAM) == bytes.fromhex("000000090000004a00000000")
    assert rv.block(rv.KEY_RFC, rv.RFC_DOMAIN, rv.RFC_STREAM, rv.RFC_FIRST) == want
    out = ctypes.create_string_buffer(64)
    twin.twin_rand_block(rv.KEY_RFC, rv.RFC_DOMAIN, rv.RFC_STREAM, rv.RFC_FIRST, out)
    assert out.raw == want


def test_addressing_twin_model(twin):
    """(domain, stream, counter) -> nonce words 13, 14, 15 and word 12, at the ends of every range."""
    out = ctypes.create_string_buffer(64)
    for key in (rv.KEY_ZERO, rv.KEY_ONES, rv.KEY_TEST):
        for domain in (0, rv.PROVE_R, rv.RHO, rv.USER, 0xFFFFFFFF):
            for stream in (0, 1, 1 << 32, rv.STREAM_MAX, 0x0123456789ABCDEF):
                for counter in (0, 1, 0xFFFFFFFE, 0xFFFFFFFF):
                    twin.twin_rand_block(key, domain, stream, counter, out)
                    assert out.raw == rv.block(key, domain, stream, counter), (domain, stream, counter)


@pytest.mark.parametrize("cname", CURVES)
def test_block_to_fr_edges(twin, cname):
    c = curve(cname)
    for name, v in rv.fr_edge_blocks(c.r):
        got = twin_fr(twin, cname, v.to_bytes(64, "little"))
        assert [int(x) for x in got] == rv.fr_boundary(v % c.r, c.r), name
        assert c.fr_dec(got) == v % c.r, name


@pytest.mark.parametrize("cname", CURVES)
def test_block_to_fr_real_output(twin, cname):
    c = curve(cname)
    for i in range(64):
        blk = rv.block(rv.KEY_TEST, rv.PROVE_R, 5, i)
        assert [int(x) for x in twin_fr(twin, cname, blk)] == rv.fr_boundary(rv.block_to_scalar(blk, c.r), c.r), i
    # the limbs next to the two 256-bit halves' boundaries, one bit at a time
    for bit in (0, 31, 32, 63, 64, 255, 256, 287, 288, 511):
        v = 1 << bit
        assert c.fr_dec(twin_fr(twin, cname, v.to_bytes(64, "little"))) == v % c.r, bit


def test_rho_mapping(twin):
    blk = rv.block(rv.KEY_TEST, rv.RHO, 9, 3)
    words = list(struct.unpack("<8Q", blk))
    assert twin_rho(twin, blk) == words == rv.block_rho(blk)  # (a real block: no zero word)
    for pos in (0, 3, 7):
        w = list(words)
        w[pos] = 0
        got = twin_rho(twin, struct.pack("<8Q", *w))
        assert got == rv.block_rho(struct.pack("<8Q", *w))
        assert got[pos] == 1 and all(got[j] == w[j] for j in range(8) if j != pos)
    assert twin_rho(twin, bytes(64)) == [1] * 8
    # a word whose low half alone is zero is not a zero word
    w = list(words)
    w[2] = 1 << 32
    assert twin_rho(twin, struct.pack("<8Q", *w))[2] == 1 << 32


def test_model_rho_layout():
    """Element j = word (first + j) mod 8 of block (first + j) div 8; a slice of a draw is the draw of the slice."""
    whole = rv.rand_rho(rv.KEY_TEST, 4, 0, 40)
    assert list(whole[:8]) == rv.block_rho(rv.block(rv.KEY_TEST, rv.RHO, 4, 0))
    assert list(rv.rand_rho(rv.KEY_TEST, 4, 5, 20)) == list(whole[5:25])


def test_symbols_declared_exported_listed():
    import groth_sahai_rs_amd as gs
    from groth_sahai_rs_amd import capi

    src = open(os.path.join(REPO, "include", "gs_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = gs.load_library()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), "not declared: " + n
        assert hasattr(lib, n), "missing export: " + n
        assert n in capi.SYMBOLS
    for name, val in (("PROVE_R", 0x0101), ("PROVE_S", 0x0102), ("PROVE_T", 0x0103), ("RERAND_R", 0x0201),
                      ("RERAND_S", 0x0202), ("RERAND_T", 0x0203), ("RHO", 0x0301), ("USER", 0x10000)):
        assert re.search(r"\bGS_RAND_%s\s*=\s*0x%04x\b" % (name, val), src, flags=re.I), "GS_RAND_" + name
        assert getattr(capi, "GS_RAND_" + name) == val == getattr(rv, name)


def test_engine_has_the_host_layer():
    from groth_sahai_rs_amd.capi import Engine

    for n in ("rand_set_key", "rand_fr", "rand_fr_dev", "rand_rho", "rand_rho_dev", "prove_batch_drawn",
              "prove_batch_drawn_dev", "prove_statement_drawn", "prove_statement_drawn_dev", "rerandomize_batch_drawn",
              "rerandomize_batch_drawn_dev", "rerandomize_statement_drawn", "rerandomize_statement_drawn_dev"):
        assert callable(getattr(Engine, n)), n
