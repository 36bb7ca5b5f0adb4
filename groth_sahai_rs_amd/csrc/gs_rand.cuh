// Keyed, counter-addressed randomness: ChaCha20 blocks (RFC 8439 section 2.3) turned into uniform Fr scalars and
// non-zero 64-bit exponents, on the device.
//
// There is no running state.  Element i of a draw is a pure function of (key, domain, stream, i):
//   state words 0..3    the "expand 32-byte k" constants
//   state words 4..11   the 32 key bytes, little-endian words
//   state word  12      the block counter
//   state words 13..15  the nonce  LE32(domain) || LE64(stream)
// so a draw does not depend on the launch shape, and a shard can draw its slice of a global array.
//   Fr:  one block per scalar, block counter = element index.  The 64 output bytes are a 512-bit little-endian
//        integer v; the scalar is v mod r (bias below 2^-256 on both curves), written in boundary (Montgomery) form.
//   rho: eight little-endian u64 per block, element j = word (j mod 8) of block (j div 8); a zero word becomes 1.
//
// The same source compiles for the host (the CPU twin of tests/): everything above the kernels is GS_HD.
#pragma once
#include "gs_field.cuh"

namespace gs {

#define GS_CHACHA_QR(a, b, c, d)        \
  x[a] += x[b];                         \
  x[d] = __builtin_rotateleft32(x[d] ^ x[a], 16); \
  x[c] += x[d];                         \
  x[b] = __builtin_rotateleft32(x[b] ^ x[c], 12); \
  x[a] += x[b];                         \
  x[d] = __builtin_rotateleft32(x[d] ^ x[a], 8);  \
  x[c] += x[d];                         \
  x[b] = __builtin_rotateleft32(x[b] ^ x[c], 7);

// out[16] = the ChaCha20 block of (key, counter, nonce words n0 n1 n2): 20 rounds, then the input state is added
GS_HD void chacha20_block(uint32_t (&out)[16], const uint32_t (&key)[8], uint32_t counter, uint32_t n0, uint32_t n1,
                          uint32_t n2) {
  uint32_t x[16];
  x[0] = 0x61707865u, x[1] = 0x3320646eu, x[2] = 0x79622d32u, x[3] = 0x6b206574u;
#pragma unroll
  for (int i = 0; i < 8; i++) x[4 + i] = key[i];
  x[12] = counter, x[13] = n0, x[14] = n1, x[15] = n2;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    GS_CHACHA_QR(0, 4, 8, 12)
    GS_CHACHA_QR(1, 5, 9, 13)
    GS_CHACHA_QR(2, 6, 10, 14)
    GS_CHACHA_QR(3, 7, 11, 15)
    GS_CHACHA_QR(0, 5, 10, 15)
    GS_CHACHA_QR(1, 6, 11, 12)
    GS_CHACHA_QR(2, 7, 8, 13)
    GS_CHACHA_QR(3, 4, 9, 14)
  }
  out[0] = x[0] + 0x61707865u, out[1] = x[1] + 0x3320646eu, out[2] = x[2] + 0x79622d32u, out[3] = x[3] + 0x6b206574u;
#pragma unroll
  for (int i = 0; i < 8; i++) out[4 + i] = x[4 + i] + key[i];
  out[12] = x[12] + counter, out[13] = x[13] + n0, out[14] = x[14] + n1, out[15] = x[15] + n2;
}
#undef GS_CHACHA_QR

// the block of element-block `counter` of (domain, stream)
GS_HD void rand_block(uint32_t (&out)[16], const uint32_t (&key)[8], uint32_t domain, uint64_t stream, uint32_t counter) {
  chacha20_block(out, key, counter, domain, (uint32_t)stream, (uint32_t)(stream >> 32));
}

// Block -> Fr.  w = 16 little-endian words of v = lo + 2^256 hi.  With R = 2^256 and the Montgomery product
// mont(a, b) = a b / R mod r:
//     v R = lo R + hi R^2 = mont(R^2 mod r, lo) + mont(R^3 mod r, hi)   (mod r).
// Input ranges of the two products: the first factor is a constant below r; the second is a RAW word string, anything
// in [0, 2^256) -- possibly >= r, and on BN254 (r of 254 bits) up to four times r.  The product computes
// (a b + M r) / R with M < R, which is below a b / R + r < a + r < 2 r < 2^256 for ANY b < R once a < r: it fits the
// 8 limbs, and mont_mul_raw's one conditional subtraction returns the canonical value.  (The CIOS form's running sum
// stays below a + r the same way; the product-scanning form's 96-bit column accumulators take any 32-bit words.)  Both
// products are canonical, so is their modular sum.
template <class C> GS_HD Fe<FrM<C>> rand_block_to_fr(const uint32_t (&w)[16]) {
  typedef FrM<C> M;
  static_assert(M::N == 8, "an Fr is 8 limbs on both curves");
  Fe<M> lo, hi, r2, r3;
#pragma unroll
  for (int j = 0; j < 8; j++) lo.v[j] = w[j], hi.v[j] = w[8 + j], r2.v[j] = M::r2(j), r3.v[j] = M::r3(j);
  return add(mul(r2, lo), mul(r3, hi));
}

// Block -> rho: the j-th little-endian u64 of a block, and the non-zero rule (bias 2^-64).  The rule is a function of
// its own so that a test can feed it the zero no real block is likely to hold.
GS_HD uint64_t rand_rho_fix(uint64_t w) { return w ? w : 1; }
GS_HD uint64_t rand_block_u64(const uint32_t (&w)[16], int j) { return (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32); }

// the library's nonce domains (include/gs_amd.h: GS_RAND_*)
constexpr uint32_t RAND_DOMAIN_RHO = 0x0301;

#if defined(__HIPCC__)
// The key is uniform across the launch: read through the constant address space (scalar loads), as the simulation
// trapdoor is.
__device__ __forceinline__ void ld_uniform_key(uint32_t (&k)[8], const uint32_t* p) {
  typedef const __attribute__((address_space(4))) uint32_t* cptr;
  cptr w = (cptr)p;
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = w[i];
}

// 32-bit add / xor / rotate and two 8-limb products: a few dozen registers.  256-thread blocks, so that the
// one-wave-per-SIMD budget of the pairing kernels (64-thread blocks, 512 VGPRs) does not apply here.
constexpr int RAND_BLOCK = 256;

// out[i] = Fr of block (first + i), i < count.  The caller has checked first + count <= 2^32.
template <class C>
__global__ void __launch_bounds__(RAND_BLOCK) k_rand_fr(size_t count, const uint32_t* key, uint32_t domain, uint64_t stream,
                                                        uint64_t first, Fe<FrM<C>>* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t k[8], w[16];
  ld_uniform_key(k, key);
  rand_block(w, k, domain, stream, (uint32_t)(first + i));
  out[i] = rand_block_to_fr<C>(w);
}

// One lane per block: lane b holds block first / 8 + b and writes those of its eight words whose global index lies in
// [first, first + count) -- the first and the last block of a draw may be partial.  nblocks = the lanes that have work.
__global__ void __launch_bounds__(RAND_BLOCK) k_rand_rho(size_t nblocks, const uint32_t* key, uint64_t stream, uint64_t first,
                                                         uint64_t count, uint64_t* out) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblocks) return;
  const uint64_t blk = first / 8 + b;  // < 2^32 (checked by the caller)
  uint32_t k[8], w[16];
  ld_uniform_key(k, key);
  rand_block(w, k, RAND_DOMAIN_RHO, stream, (uint32_t)blk);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint64_t g = blk * 8 + j;
    if (g >= first && g - first < count) out[g - first] = rand_rho_fix(rand_block_u64(w, j));
  }
}
#endif  // __HIPCC__

}  // namespace gs
