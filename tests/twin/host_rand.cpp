// CPU twin of the device generator: csrc/gs_rand.cuh compiled for the host with clang++ (no HIP), behind a tiny C ABI
// so that pytest can hold the block function and the two maps against the Python model and the OpenSSL fixture
// without a GPU.  Test infrastructure only -- never loaded by the product.
#include <string.h>
#include "../../groth_sahai_rs_amd/csrc/gs_params_bls12_381.h"
#include "../../groth_sahai_rs_amd/csrc/gs_params_bn254.h"
#include "../../groth_sahai_rs_amd/csrc/gs_rand.cuh"

using namespace gs;

static void words_of(uint32_t (&w)[16], const uint8_t* b) {
  for (int i = 0; i < 16; i++)
    w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
static void bytes_of(uint8_t* b, const uint32_t (&w)[16]) {
  for (int i = 0; i < 16; i++)
    for (int k = 0; k < 4; k++) b[4 * i + k] = (uint8_t)(w[i] >> (8 * k));
}
static void key_of(uint32_t (&k)[8], const uint8_t* key) {
  for (int i = 0; i < 8; i++)
    k[i] = (uint32_t)key[4 * i] | ((uint32_t)key[4 * i + 1] << 8) | ((uint32_t)key[4 * i + 2] << 16) | ((uint32_t)key[4 * i + 3] << 24);
}
template <class C> static void to_fr(const uint8_t* block, uint64_t* out) {
  uint32_t w[16];
  words_of(w, block);
  const Fe<FrM<C>> r = rand_block_to_fr<C>(w);
  for (int i = 0; i < 4; i++) out[i] = (uint64_t)r.v[2 * i] | ((uint64_t)r.v[2 * i + 1] << 32);
}

extern "C" {
// the raw block function: nonce as its three little-endian words
void twin_chacha20_block(const uint8_t* key, uint32_t counter, const uint8_t* nonce12, uint8_t* out64) {
  uint32_t k[8], w[16], n[3];
  key_of(k, key);
  for (int i = 0; i < 3; i++)
    n[i] = (uint32_t)nonce12[4 * i] | ((uint32_t)nonce12[4 * i + 1] << 8) | ((uint32_t)nonce12[4 * i + 2] << 16) |
           ((uint32_t)nonce12[4 * i + 3] << 24);
  chacha20_block(w, k, counter, n[0], n[1], n[2]);
  bytes_of(out64, w);
}
// the generator's addressing: (domain, stream, block counter)
void twin_rand_block(const uint8_t* key, uint32_t domain, uint64_t stream, uint32_t counter, uint8_t* out64) {
  uint32_t k[8], w[16];
  key_of(k, key);
  rand_block(w, k, domain, stream, counter);
  bytes_of(out64, w);
}
void twin_block_to_fr_bls12_381(const uint8_t* block, uint64_t* out) { to_fr<Bls12_381>(block, out); }
void twin_block_to_fr_bn254(const uint8_t* block, uint64_t* out) { to_fr<Bn254>(block, out); }
// the eight exponents of a block, through the two GS_HD functions the kernel uses
void twin_block_rho(const uint8_t* block, uint64_t* out8) {
  uint32_t w[16];
  words_of(w, block);
  for (int j = 0; j < 8; j++) out8[j] = rand_rho_fix(rand_block_u64(w, j));
}
}
