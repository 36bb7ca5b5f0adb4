// Statement::verify_rlc (include/gs_amd.hpp) on the GPU through the C ABI: a mixed-type statement with two equations
// per type over ONE list of variables is accepted by the combined check exactly when Statement::verify accepts every
// equation -- true for the honest proof, false once one pi is exchanged with another equation's.
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

struct U64Rng : MixRng {  // a generator with a 64-bit draw of its own: verify_rlc takes its exponents from there
  size_t words = 0;
  uint64_t u64() {
    words++;
    return words == 1 ? 0 : next();  // the first draw is zero: it must be drawn again, never used
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

constexpr size_t E = 2;  // equations per type

template <class A1, class A2, class AT, EquType TY>
static std::vector<Equation<A1, A2, AT, TY>> equations(std::ifstream& f, size_t m, size_t n) {
  Bytes A = section(f), B = section(f), G = section(f), T = section(f);
  auto a = split<A1>(A, E * n);
  auto b = split<A2>(B, E * m);
  auto g = split<Fr>(G, E * m * n);
  auto t = split<AT>(T, E);
  std::vector<Equation<A1, A2, AT, TY>> out(E);
  for (size_t e = 0; e < E; e++) {
    out[e].a_consts.assign(a.begin() + e * n, a.begin() + (e + 1) * n);
    out[e].b_consts.assign(b.begin() + e * m, b.begin() + (e + 1) * m);
    out[e].gamma.resize(m);
    for (size_t i = 0; i < m; i++)
      out[e].gamma[i].assign(g.begin() + (e * m + i) * n, g.begin() + (e * m + i + 1) * n);
    out[e].target = t[e];
  }
  return out;
}

static bool all_true(const std::vector<bool>& v) {
  for (bool b : v)
    if (!b) return false;
  return true;
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
  StatementVars vars;
  vars.xg = split<G1Affine>(xg, mg);
  vars.yg = split<G2Affine>(yg, ng);
  vars.xs = split<Fr>(xs, ms);
  vars.ys = split<Fr>(ys, ns);
  auto ppe = equations<G1Affine, G2Affine, GT, EquType::PairingProduct>(f, mg, ng);
  auto ms1 = equations<G1Affine, Fr, G1Affine, EquType::MultiScalarG1>(f, mg, ns);
  auto ms2 = equations<Fr, G2Affine, G2Affine, EquType::MultiScalarG2>(f, ms, ng);
  auto qua = equations<Fr, Fr, Fr, EquType::Quadratic>(f, ms, ns);
  Statement st;  // the types interleaved: equations 0..3 are the first of each type, 4..7 the second
  for (size_t e = 0; e < E; e++) {
    st.push(ppe[e]);
    st.push(ms1[e]);
    st.push(ms2[e]);
    st.push(qua[e]);
  }
  CHECK(st.size() == 4 * E);
  MixRng prover{0x57A7E};
  StatementProof proof = st.commit_and_prove(vars, crs, prover);
  std::vector<bool> each = st.verify(proof, crs);
  CHECK(each.size() == st.size() && all_true(each));
  MixRng rho{0xC0FFEE};
  CHECK(st.verify_rlc(proof, crs, rho));
  CHECK(rho.draws == 4 * st.size());  // one 64-bit exponent per cell of every equation (no zero drawn by this stream)
  CHECK(st.verify_rlc(proof, crs, rho));  // fresh exponents, same verdict
  U64Rng words{{0xBEEF}};
  CHECK(st.verify_rlc(proof, crs, words));
  CHECK(words.draws == 0 && words.words == 4 * st.size() + 1);  // u64() alone, the zero drawn again
  // one pi exchanged with the other equation's of its type, type by type: rejected, in agreement with verify
  for (size_t ty = 0; ty < 4; ty++) {
    StatementProof bad = proof;
    std::swap(bad.equ_proofs[ty].pi, bad.equ_proofs[4 + ty].pi);
    std::vector<bool> v = st.verify(bad, crs);
    CHECK(!v[ty] && !v[4 + ty]);
    for (size_t i = 0; i < v.size(); i++) CHECK(v[i] == (i != ty && i != 4 + ty));
    CHECK(st.verify_rlc(bad, crs, rho) == all_true(v));
    CHECK(!st.verify_rlc(bad, crs, rho));
  }
  // the reference's shape asserts hold for the combined check too
  bool threw = false;
  try {
    StatementProof shortp = proof;
    shortp.equ_proofs[1].pi.pop_back();
    st.verify_rlc(shortp, crs, rho);
  } catch (const Panic&) {
    threw = true;
  }
  CHECK(threw);
  std::printf("OK %d\n", checks);
  return 0;
}
