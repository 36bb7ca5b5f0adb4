// DeviceRng (include/gs_amd.hpp) on the GPU through the C ABI: commit_and_prove -> verify -> rerandomize -> verify with
// R, S, T drawn on the device; the randomness the objects carry is the model's (tests/randvec.py), and the ordinary
// entries driven by it give the same bytes.
// Input: argv[1] the case blob of tests/test_gpu_cpp_host.py (u32 curve, type, m, n; then length-prefixed (u64)
//   sections u0 u1 v0 v1 g1 g2 gt X Y A B Gamma target ...; the sections after target are not read);
//   argv[2] the model's draws as length-prefixed sections: key (32 bytes), R S T of GS_RAND_PROVE_* on stream 0,
//   R' S' of GS_RAND_RERAND_R/S on stream 1, and R S T of a two-equation statement on stream 2.
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
static ReplayRng replay(std::initializer_list<const Matrix<Fr>*> mats) {
  ReplayRng r;
  for (const Matrix<Fr>* mt : mats)
    for (const auto& row : *mt) r.q.insert(r.q.end(), row.begin(), row.end());
  return r;
}

static Bytes section(std::ifstream& f) {
  uint64_t n = 0;
  f.read((char*)&n, 8);
  Bytes b(n);
  f.read((char*)b.data(), n);
  if (!f) {
    std::fprintf(stderr, "short input file\n");
    std::exit(2);
  }
  return b;
}

static bool same(const CProof& a, const CProof& b) {
  const EquProof &p = a.equ_proofs[0], &q = b.equ_proofs[0];
  return cat(a.xcoms.coms) == cat(b.xcoms.coms) && cat(a.ycoms.coms) == cat(b.ycoms.coms) && cat(p.pi) == cat(q.pi) &&
         cat(p.theta) == cat(q.theta);
}

struct Model {
  Bytes key, R, S, T, R1, S1, sR, sS, sT;
};

template <class A1, class A2, class AT, EquType TY>
static void run(const CRS& crs, uint32_t m, uint32_t n, const Bytes& X, const Bytes& Y, const Bytes& A, const Bytes& B,
                const Bytes& G, const Bytes& tgt, const Model& md) {
  using Equ = Equation<A1, A2, AT, TY>;
  Equ equ;
  equ.a_consts = split<A1>(A, n);
  equ.b_consts = split<A2>(B, m);
  auto gflat = split<Fr>(G, (size_t)m * n);
  equ.gamma.resize(m);
  for (uint32_t i = 0; i < m; i++) equ.gamma[i].assign(gflat.begin() + i * n, gflat.begin() + (i + 1) * n);
  equ.target.v = tgt;
  auto xvars = split<A1>(X, m);
  auto yvars = split<A2>(Y, n);

  DeviceRng rng(crs, md.key);
  CProof proof = equ.commit_and_prove(xvars, yvars, crs, rng);
  CHECK(rng.stream == 1);
  CHECK(equ.verify(proof, crs));
  // the carried randomness is the model's draw of stream 0 ...
  CHECK(cat(proof.xcoms.rand) == md.R && cat(proof.ycoms.rand) == md.S && cat(proof.equ_proofs[0].rand) == md.T);
  CHECK(proof.xcoms.rand.size() == m && proof.xcoms.rand[0].size() == Equ::KX);
  CHECK(proof.ycoms.rand.size() == n && proof.ycoms.rand[0].size() == Equ::KY);
  CHECK(proof.equ_proofs[0].rand.size() == Equ::KY && proof.equ_proofs[0].rand[0].size() == Equ::KX);
  // ... and the proof's: the ordinary prover on it gives the same bytes
  ReplayRng r0 = replay({&proof.xcoms.rand, &proof.ycoms.rand, &proof.equ_proofs[0].rand});
  CHECK(same(equ.commit_and_prove(xvars, yvars, crs, r0), proof));

  CProof q = equ.rerandomize(proof, crs, rng);
  CHECK(rng.stream == 2);
  CHECK(equ.verify(q, crs));
  CHECK(cat(q.xcoms.coms) != cat(proof.xcoms.coms) && cat(q.equ_proofs[0].pi) != cat(proof.equ_proofs[0].pi));
  // q carries R + R', S + S' with R', S' the model's RERAND draws of stream 1, and T'' such that the ordinary prover
  // reproduces q
  const int cv = crs.ctx->curve_id;
  CHECK(cat(q.xcoms.rand) == cat(detail::fr_mat_add(proof.xcoms.rand, detail::fr_matrix(md.R1, m, Equ::KX), cv)));
  CHECK(cat(q.ycoms.rand) == cat(detail::fr_mat_add(proof.ycoms.rand, detail::fr_matrix(md.S1, n, Equ::KY), cv)));
  ReplayRng r1 = replay({&q.xcoms.rand, &q.ycoms.rand, &q.equ_proofs[0].rand});
  CHECK(same(equ.commit_and_prove(xvars, yvars, crs, r1), q));

  // a statement of two copies of the equation: R, S once, T per equation, all the model's draws of stream 2
  Statement st;
  st.push(equ);
  st.push(equ);
  StatementVars v;
  if constexpr (Equ::KX == 2) v.xg = xvars; else v.xs = xvars;
  if constexpr (Equ::KY == 2) v.yg = yvars; else v.ys = yvars;
  StatementProof sp = st.commit_and_prove(v, crs, rng);
  CHECK(rng.stream == 3);
  const std::vector<bool> oks = st.verify(sp, crs);
  CHECK(oks.size() == 2 && oks[0] && oks[1]);
  const Commit1& cx = Equ::KX == 2 ? sp.com_xg : sp.com_xs;
  const Commit2& cy = Equ::KY == 2 ? sp.com_yg : sp.com_ys;
  CHECK(cat(cx.rand) == md.sR && cat(cy.rand) == md.sS);
  Bytes ts = cat(sp.equ_proofs[0].rand), t1 = cat(sp.equ_proofs[1].rand);
  ts.insert(ts.end(), t1.begin(), t1.end());
  CHECK(ts == md.sT);

  // a short key is refused before anything is installed
  bool threw = false;
  try {
    DeviceRng bad(crs, Bytes(31));
  } catch (const Panic&) {
    threw = true;
  }
  CHECK(threw);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  uint32_t hdr[4];
  f.read((char*)hdr, sizeof hdr);
  uint32_t curve = hdr[0], ty = hdr[1], m = hdr[2], n = hdr[3];
  Bytes u0 = section(f), u1 = section(f), v0 = section(f), v1 = section(f), g1 = section(f), g2 = section(f),
        gt = section(f), X = section(f), Y = section(f), A = section(f), B = section(f), G = section(f),
        tgt = section(f);
  std::ifstream g(argv[2], std::ios::binary);
  Model md;
  md.key = section(g), md.R = section(g), md.S = section(g), md.T = section(g), md.R1 = section(g), md.S1 = section(g);
  md.sR = section(g), md.sS = section(g), md.sT = section(g);
  CRS crs({Com1{u0}, Com1{u1}}, {Com2{v0}, Com2{v1}}, G1Affine{g1}, G2Affine{g2}, GT{gt}, (int)curve, 0);
  switch (ty) {
    case 0: run<G1Affine, G2Affine, GT, EquType::PairingProduct>(crs, m, n, X, Y, A, B, G, tgt, md); break;
    case 1: run<G1Affine, Fr, G1Affine, EquType::MultiScalarG1>(crs, m, n, X, Y, A, B, G, tgt, md); break;
    case 2: run<Fr, G2Affine, G2Affine, EquType::MultiScalarG2>(crs, m, n, X, Y, A, B, G, tgt, md); break;
    case 3: run<Fr, Fr, Fr, EquType::Quadratic>(crs, m, n, X, Y, A, B, G, tgt, md); break;
    default: return 2;
  }
  std::printf("OK %d\n", checks);
  return 0;
}
