// Equation::verify_rlc_many (include/gs_amd.hpp) on the GPU through the C ABI: five showings of one proven equation --
// the proof and four rerandomizations of it -- are accepted by ONE combined check (gs_verify_equation_rlc), and rejected
// once the pi of one showing is exchanged with another showing's, for each of the four equation types.
// Input: the blob of tests/test_gpu_stmt_rlc_cpp.py (u32 curve, mg, ng, ms, ns; then length-prefixed (u64) sections
//   u0 u1 v0 v1 g1 g2 gt xg yg xs ys, then A B Gamma target of the two equations of type 0, 1, 2, 3).
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

constexpr size_t E = 2;  // equations per type in the blob; the first of each type is used

template <class A1, class A2, class AT, EquType TY>
static Equation<A1, A2, AT, TY> first_equation(std::ifstream& f, size_t m, size_t n) {
  Bytes A = section(f), B = section(f), G = section(f), T = section(f);
  auto a = split<A1>(A, E * n);
  auto b = split<A2>(B, E * m);
  auto g = split<Fr>(G, E * m * n);
  auto t = split<AT>(T, E);
  Equation<A1, A2, AT, TY> out;
  out.a_consts.assign(a.begin(), a.begin() + n);
  out.b_consts.assign(b.begin(), b.begin() + m);
  out.gamma.resize(m);
  for (size_t i = 0; i < m; i++) out.gamma[i].assign(g.begin() + i * n, g.begin() + (i + 1) * n);
  out.target = t[0];
  return out;
}

template <class EQ, class X, class Y>
static void showings(const EQ& equ, const std::vector<X>& xvars, const std::vector<Y>& yvars, const CRS& crs) {
  MixRng prover{0x5E0111};
  std::vector<CProof> shown{equ.commit_and_prove(xvars, yvars, crs, prover)};
  for (int k = 0; k < 4; k++) shown.push_back(equ.rerandomize(shown[0], crs, prover));
  for (const CProof& cp : shown) CHECK(equ.verify(cp, crs));
  MixRng rho{0xC0FFEE};
  CHECK(equ.verify_rlc_many(shown, crs, rho));
  CHECK(rho.draws == 4 * shown.size());  // one 64-bit exponent per cell of every proof (no zero drawn by this stream)
  CHECK(equ.verify_rlc_many(shown, crs, rho));  // fresh exponents, same verdict
  CHECK(equ.verify_rlc_many(std::vector<CProof>{shown[3]}, crs, rho));
  std::vector<CProof> bad = shown;
  std::swap(bad[1].equ_proofs[0].pi, bad[4].equ_proofs[0].pi);
  CHECK(!equ.verify(bad[1], crs) && !equ.verify(bad[4], crs));
  CHECK(!equ.verify_rlc_many(bad, crs, rho));
  bool threw = false;
  try {
    std::vector<CProof> shortp = shown;
    shortp[2].equ_proofs[0].theta.pop_back();
    equ.verify_rlc_many(shortp, crs, rho);
  } catch (const Panic&) {
    threw = true;
  }
  CHECK(threw);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  uint32_t hdr[5];
  f.read((char*)hdr, sizeof hdr);
  const uint32_t curve = hdr[0], mg = hdr[1], ng = hdr[2], ms = hdr[3], ns = hdr[4];
  Bytes u0 = section(f), u1 = section(f), v0 = section(f), v1 = section(f), g1 = section(f), g2 = section(f),
        gt = section(f), xg = section(f), yg = section(f), xs = section(f), ys = section(f);
  CRS crs({Com1{u0}, Com1{u1}}, {Com2{v0}, Com2{v1}}, G1Affine{g1}, G2Affine{g2}, GT{gt}, (int)curve, 0);
  auto vxg = split<G1Affine>(xg, mg);
  auto vyg = split<G2Affine>(yg, ng);
  auto vxs = split<Fr>(xs, ms);
  auto vys = split<Fr>(ys, ns);
  auto ppe = first_equation<G1Affine, G2Affine, GT, EquType::PairingProduct>(f, mg, ng);
  auto ms1 = first_equation<G1Affine, Fr, G1Affine, EquType::MultiScalarG1>(f, mg, ns);
  auto ms2 = first_equation<Fr, G2Affine, G2Affine, EquType::MultiScalarG2>(f, ms, ng);
  auto qua = first_equation<Fr, Fr, Fr, EquType::Quadratic>(f, ms, ns);
  showings(ppe, vxg, vyg, crs);
  showings(ms1, vxg, vys, crs);
  showings(ms2, vxs, vyg, crs);
  showings(qua, vxs, vys, crs);
  std::printf("OK %d\n", checks);
  return 0;
}
