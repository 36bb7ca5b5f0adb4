"""Pure-Python model of the device generator (csrc/gs_rand.cuh): the ChaCha20 block of RFC 8439 section 2.3, block ->
Fr and block -> rho, the layout model of the drawn entries, and the named edge inputs the CPU and GPU tests share.

Nothing here is taken from the code under test: the block function is written from the RFC, the maps from the text
of include/gs_amd.h ("randomness drawn on the device")."""
import struct

import numpy as np

M32 = 0xFFFFFFFF
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"

# the library's domains (include/gs_amd.h)
PROVE_R, PROVE_S, PROVE_T = 0x0101, 0x0102, 0x0103
RERAND_R, RERAND_S, RERAND_T = 0x0201, 0x0202, 0x0203
RHO = 0x0301
USER = 0x10000


def _rotl(v, n):
    return ((v << n) & M32) | (v >> (32 - n))


def _qr(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32
    x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32
    x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32
    x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32
    x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_block(key, counter, nonce):
    """key: 32 bytes, counter: 0 .. 2^32 - 1, nonce: 12 bytes -> the 64 bytes of the block."""
    assert len(key) == 32 and len(nonce) == 12 and 0 <= counter <= M32
    init = list(SIGMA) + list(struct.unpack("<8I", key)) + [counter] + list(struct.unpack("<3I", nonce))
    x = list(init)
    for _ in range(10):
        _qr(x, 0, 4, 8, 12)
        _qr(x, 1, 5, 9, 13)
        _qr(x, 2, 6, 10, 14)
        _qr(x, 3, 7, 11, 15)
        _qr(x, 0, 5, 10, 15)
        _qr(x, 1, 6, 11, 12)
        _qr(x, 2, 7, 8, 13)
        _qr(x, 3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & M32 for a, b in zip(x, init)])


def nonce_of(domain, stream):
    """LE32(domain) || LE64(stream): domain is state word 13, the halves of stream words 14 and 15."""
    return struct.pack("<IQ", domain, stream)


def block(key, domain, stream, counter):
    return chacha20_block(key, counter, nonce_of(domain, stream))


def block_to_scalar(blk, r):
    """The 64 bytes as a 512-bit little-endian integer, mod r."""
    return int.from_bytes(blk, "little") % r


def fr_boundary(x, r):
    """4 u64 limbs of x 2^256 mod r."""
    v = x * (1 << 256) % r
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def rand_fr_ints(key, r, domain, stream, first, count):
    assert first + count <= 1 << 32
    return [block_to_scalar(block(key, domain, stream, first + i), r) for i in range(count)]


def rand_fr(key, r, domain, stream, first, count):
    """What gs_rand_fr writes: uint64 array [count][4]."""
    return np.array([fr_boundary(x, r) for x in rand_fr_ints(key, r, domain, stream, first, count)],
                    dtype=np.uint64).reshape(count, 4)


def rho_fix(w):
    return w if w else 1


def block_rho(blk):
    """The eight exponents of one block."""
    return [rho_fix(w) for w in struct.unpack("<8Q", blk)]


def rand_rho(key, stream, first, count):
    """What gs_rand_rho writes: element j = word (first + j) mod 8 of block (first + j) div 8."""
    assert (first + count + 7) // 8 <= 1 << 32
    cache, out = {}, []
    for g in range(first, first + count):
        b = g // 8
        if b not in cache:
            cache[b] = block_rho(block(key, RHO, stream, b))
        out.append(cache[b][g % 8])
    return np.array(out, dtype=np.uint64)


# ---- the drawn entries' layout -------------------------------------------------------------------------------------
def shape(ty):
    xg, yg = ty in (0, 1), ty in (0, 2)
    return (2 if xg else 1), (2 if yg else 1)


def drawn_rst(key, r, ty, N, m, n, stream, shared=False, rerand=False):
    """R, S, T of a drawn entry, as flat uint64 arrays: element index = flat array index, each array its own domain
    from counter 0.  shared: a Statement -- R[m][kx], S[n][ky] once, T[N][ky][kx]."""
    kx, ky = shape(ty)
    V = 1 if shared else N
    dR, dS, dT = (RERAND_R, RERAND_S, RERAND_T) if rerand else (PROVE_R, PROVE_S, PROVE_T)
    return (rand_fr(key, r, dR, stream, 0, V * m * kx).reshape(-1),
            rand_fr(key, r, dS, stream, 0, V * n * ky).reshape(-1),
            rand_fr(key, r, dT, stream, 0, N * ky * kx).reshape(-1))


# ---- named inputs ---------------------------------------------------------------------------------------------------
KEY_ZERO = bytes(32)
KEY_ONES = b"\xff" * 32
KEY_RFC = bytes(range(32))  # RFC 8439 section 2.3.2
KEY_TEST = bytes((37 * i + 11) & 0xFF for i in range(32))
# RFC 8439 section 2.3.2: nonce 00 00 00 09 00 00 00 4a 00 00 00 00, counter 1
RFC_DOMAIN, RFC_STREAM, RFC_FIRST = 0x09000000, 0x4A000000, 1
RFC_BLOCK_HEX = (
    "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
    "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
STREAM_MAX = (1 << 64) - 1


def fr_edge_blocks(r):
    """(name, 512-bit integer) pairs every block -> Fr implementation must reduce correctly."""
    return [("zero", 0), ("all_ones", (1 << 512) - 1), ("r-1", r - 1), ("r", r), ("r+1", r + 1),
            ("2^256-1", (1 << 256) - 1), ("2^256", 1 << 256), ("2^256(r-1)+(r-1)", (1 << 256) * (r - 1) + (r - 1))]
