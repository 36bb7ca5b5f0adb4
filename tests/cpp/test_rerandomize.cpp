// Equation::rerandomize (include/gs_amd.hpp) on the GPU through the C ABI: a rerandomized proof verifies, differs from
// its input, carries the combined randomness, and equals commit_and_prove driven by that randomness byte for byte;
// an invalid proof stays invalid; a proof without its randomness is rerandomized all the same.
// Input: the case blob of tests/test_gpu_cpp_host.py (u32 curve, type, m, n; then length-prefixed (u64) sections
//   u0 u1 v0 v1 g1 g2 gt X Y A B Gamma target R S T ...; the sections after T are not read).
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

struct ReplayRng {  // hands out recorded draws in order
  std::vector<Fr> q;
  size_t i = 0;
  Fr fr() {
    if (i >= q.size()) {
      std::fprintf(stderr, "rng exhausted\n");
      std::exit(1);
    }
    return q[i++];
  }
};
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

static bool same(const CProof& a, const CProof& b) {
  const EquProof &p = a.equ_proofs[0], &q = b.equ_proofs[0];
  return cat(a.xcoms.coms) == cat(b.xcoms.coms) && cat(a.ycoms.coms) == cat(b.ycoms.coms) && cat(p.pi) == cat(q.pi) &&
         cat(p.theta) == cat(q.theta);
}

template <class A1, class A2, class AT, EquType TY>
static void run(const CRS& crs, uint32_t m, uint32_t n, const Bytes& X, const Bytes& Y, const Bytes& A, const Bytes& B,
                const Bytes& G, const Bytes& tgt, const Bytes& R, const Bytes& S, const Bytes& T) {
  using Equ = Equation<A1, A2, AT, TY>;
  const size_t fr = crs.ctx->sz[1];
  Equ equ;
  equ.a_consts = split<A1>(A, n);
  equ.b_consts = split<A2>(B, m);
  auto gflat = split<Fr>(G, (size_t)m * n);
  equ.gamma.resize(m);
  for (uint32_t i = 0; i < m; i++) equ.gamma[i].assign(gflat.begin() + i * n, gflat.begin() + (i + 1) * n);
  equ.target.v = tgt;
  auto xvars = split<A1>(X, m);
  auto yvars = split<A2>(Y, n);
  ReplayRng rng;
  for (const Bytes* p : {&R, &S, &T}) {
    auto v = split<Fr>(*p, p->size() / fr);
    rng.q.insert(rng.q.end(), v.begin(), v.end());
  }
  CProof proof = equ.commit_and_prove(xvars, yvars, crs, rng);
  CHECK(equ.verify(proof, crs));

  MixRng mix{0x5EEDull + (uint64_t)TY};
  CProof q = equ.rerandomize(proof, crs, mix);
  CHECK(mix.draws == m * Equ::KX + n * Equ::KY + Equ::KY * Equ::KX);  // R', S', T' and nothing else
  CHECK(q.equ_proofs.size() == 1 && q.equ_proofs[0].equ_type == TY);
  CHECK(q.equ_proofs[0].pi.size() == Equ::KX && q.equ_proofs[0].theta.size() == Equ::KY);
  CHECK(equ.verify(q, crs));
  CHECK(cat(q.xcoms.coms) != cat(proof.xcoms.coms) && cat(q.equ_proofs[0].pi) != cat(proof.equ_proofs[0].pi));
  // the combined randomness drives commit_and_prove to the same bytes
  ReplayRng r2;
  for (const Matrix<Fr>* mt : {&q.xcoms.rand, &q.ycoms.rand, &q.equ_proofs[0].rand})
    for (const auto& row : *mt) r2.q.insert(r2.q.end(), row.begin(), row.end());
  CHECK(r2.q.size() == mix.draws);
  CProof fresh = equ.commit_and_prove(xvars, yvars, crs, r2);
  CHECK(same(fresh, q));
  // twice in a row: the randomness accumulates and the bytes still match
  CProof q2 = equ.rerandomize(q, crs, mix);
  CHECK(equ.verify(q2, crs));
  ReplayRng r3;
  for (const Matrix<Fr>* mt : {&q2.xcoms.rand, &q2.ycoms.rand, &q2.equ_proofs[0].rand})
    for (const auto& row : *mt) r3.q.insert(r3.q.end(), row.begin(), row.end());
  CHECK(same(equ.commit_and_prove(xvars, yvars, crs, r3), q2));

  // a proof that arrives without its randomness (what a third party holds)
  CProof bare = proof;
  bare.xcoms.rand.clear();
  bare.ycoms.rand.clear();
  bare.equ_proofs[0].rand.clear();
  MixRng mix2{0x5EEDull + (uint64_t)TY};
  CProof qb = equ.rerandomize(bare, crs, mix2);
  CHECK(same(qb, q) && qb.xcoms.rand.empty() && qb.equ_proofs[0].rand.empty());
  CHECK(equ.verify(qb, crs));

  // an invalid proof stays invalid
  CProof bad = proof;
  bad.equ_proofs[0].theta[0] = proof.xcoms.coms[0];
  CHECK(!equ.verify(bad, crs));
  CProof qbad = equ.rerandomize(bad, crs, mix);
  CHECK(!equ.verify(qbad, crs));

  // the reference's shape asserts
  CProof short_pi = proof;
  short_pi.equ_proofs[0].pi.pop_back();
  bool threw = false;
  try {
    equ.rerandomize(short_pi, crs, mix);
  } catch (const Panic&) {
    threw = true;
  }
  CHECK(threw);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  uint32_t hdr[4];
  f.read((char*)hdr, sizeof hdr);
  uint32_t curve = hdr[0], ty = hdr[1], m = hdr[2], n = hdr[3];
  Bytes u0 = section(f), u1 = section(f), v0 = section(f), v1 = section(f), g1 = section(f), g2 = section(f),
        gt = section(f), X = section(f), Y = section(f), A = section(f), B = section(f), G = section(f),
        tgt = section(f), R = section(f), S = section(f), T = section(f);
  CRS crs({Com1{u0}, Com1{u1}}, {Com2{v0}, Com2{v1}}, G1Affine{g1}, G2Affine{g2}, GT{gt}, (int)curve, 0);
  switch (ty) {
    case 0: run<G1Affine, G2Affine, GT, EquType::PairingProduct>(crs, m, n, X, Y, A, B, G, tgt, R, S, T); break;
    case 1: run<G1Affine, Fr, G1Affine, EquType::MultiScalarG1>(crs, m, n, X, Y, A, B, G, tgt, R, S, T); break;
    case 2: run<Fr, G2Affine, G2Affine, EquType::MultiScalarG2>(crs, m, n, X, Y, A, B, G, tgt, R, S, T); break;
    case 3: run<Fr, Fr, Fr, EquType::Quadratic>(crs, m, n, X, Y, A, B, G, tgt, R, S, T); break;
    default: return 2;
  }
  std::printf("OK %d\n", checks);
  return 0;
}
