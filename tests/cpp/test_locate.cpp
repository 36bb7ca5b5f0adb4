// verify_batch_locate (include/gs_amd.hpp) on the GPU through the C ABI: four pairing-product equations, each with a
// CProof of its own; honest proofs are all accepted, and once the pi of one proof is replaced by another proof's, the
// verdicts are {1, 0, 1, 1} -- what Equation::verify says entry by entry.
// Input: the blob of tests/test_gpu_stmt_rlc_cpp.py (u32 curve, mg, ng, ms, ns; then length-prefixed (u64) sections
//   u0 u1 v0 v1 g1 g2 gt xg yg xs ys, then A B Gamma target of the two equations of type 0; the rest is not read).
// Exit code 0 and "OK <checks>" on success.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "gs_amd.hpp"

using namespace gs_amd;

static int checks = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                    \
    }                                                                  \
    checks++;                                                          \
  } while (0)

struct MixRng {  // splitmix64; the top limb kept below 2^60 so that every draw is a valid scalar (< r) of both curves
  uint64_t s;
  size_t draws = 0;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  Fr fr() {
    uint64_t v[4] = {next(), next(), next(), next() >> 4};
    Fr f;
    f.v.resize(32);
    std::memcpy(f.v.data(), v, 32);
    draws++;
    return f;
  }
};

struct U64Rng : MixRng {  // a generator with a 64-bit draw of its own; its first draw is zero and must be drawn again
  size_t words = 0;
  uint64_t u64() {
    words++;
    return words == 1 ? 0 : next();
  }
};

static Bytes section(std::ifstream& f) {
  uint64_t n = 0;
  f.read((char*)&n, 8);
  Bytes b(n);
  f.read((char*)b.data(), n);
  if (!f) {
    std::fprintf(stderr, "short case file\n");
    std::exit(2);
  }
  return b;
}

typedef Equation<G1Affine, G2Affine, GT, EquType::PairingProduct> Ppe;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  uint32_t hdr[5];
  f.read((char*)hdr, sizeof hdr);
  const uint32_t curve = hdr[0], m = hdr[1], n = hdr[2];
  Bytes u0 = section(f), u1 = section(f), v0 = section(f), v1 = section(f), g1 = section(f), g2 = section(f),
        gt = section(f), xg = section(f), yg = section(f), xs = section(f), ys = section(f);
  CRS crs({Com1{u0}, Com1{u1}}, {Com2{v0}, Com2{v1}}, G1Affine{g1}, G2Affine{g2}, GT{gt}, (int)curve, 0);
  std::vector<G1Affine> xvars = split<G1Affine>(xg, m);
  std::vector<G2Affine> yvars = split<G2Affine>(yg, n);
  Bytes A = section(f), B = section(f), G = section(f), T = section(f);
  auto a = split<G1Affine>(A, 2 * n);
  auto b = split<G2Affine>(B, 2 * m);
  auto g = split<Fr>(G, 2 * m * n);
  auto t = split<GT>(T, 2);
  // four equations: the blob's two, each taken twice; every one gets commitments and a proof of its own
  std::vector<Ppe> equs(4);
  std::vector<CProof> proofs;
  MixRng prover{0x10CA7E};
  for (size_t k = 0; k < 4; k++) {
    const size_t e = k & 1;
    equs[k].a_consts.assign(a.begin() + e * n, a.begin() + (e + 1) * n);
    equs[k].b_consts.assign(b.begin() + e * m, b.begin() + (e + 1) * m);
    equs[k].gamma.resize(m);
    for (size_t i = 0; i < m; i++) equs[k].gamma[i].assign(g.begin() + (e * m + i) * n, g.begin() + (e * m + i + 1) * n);
    equs[k].target = t[e];
    proofs.push_back(equs[k].commit_and_prove(xvars, yvars, crs, prover));
    CHECK(equs[k].verify(proofs[k], crs));
  }
  MixRng rho{0xC0FFEE};
  std::vector<bool> ok = verify_batch_locate(equs, proofs, crs, rho);
  CHECK(ok.size() == 4 && ok[0] && ok[1] && ok[2] && ok[3]);
  CHECK(rho.draws == 4 * 4);  // one 64-bit exponent per cell of every equation (no zero drawn by this stream)
  U64Rng words{{0xBEEF}};
  ok = verify_batch_locate(equs, proofs, crs, words);
  CHECK(ok[0] && ok[1] && ok[2] && ok[3]);
  CHECK(words.draws == 0 && words.words == 4 * 4 + 1);  // u64() alone, the zero drawn again
  // proof 1 gets the pi of proof 3 (the same equation under other commitments): exactly that entry fails
  std::vector<CProof> bad = proofs;
  bad[1].equ_proofs[0].pi = proofs[3].equ_proofs[0].pi;
  std::vector<bool> each;
  for (size_t k = 0; k < 4; k++) each.push_back(equs[k].verify(bad[k], crs));
  CHECK(each[0] && !each[1] && each[2] && each[3]);
  ok = verify_batch_locate(equs, bad, crs, rho);
  CHECK(ok == each);
  // two bad entries, first and last
  bad[3].equ_proofs[0].theta = proofs[1].equ_proofs[0].theta;
  bad[0].equ_proofs[0].pi = proofs[2].equ_proofs[0].pi;
  each.clear();
  for (size_t k = 0; k < 4; k++) each.push_back(equs[k].verify(bad[k], crs));
  CHECK(!each[0] && !each[1] && each[2] && !each[3]);
  CHECK(verify_batch_locate(equs, bad, crs, rho) == each);
  // the reference's shape asserts hold here too
  bool threw = false;
  try {
    std::vector<CProof> shortp = proofs;
    shortp[2].equ_proofs[0].pi.pop_back();
    verify_batch_locate(equs, shortp, crs, rho);
  } catch (const Panic&) {
    threw = true;
  }
  CHECK(threw);
  std::printf("OK %d\n", checks);
  return 0;
}
