// CRS::generate_hiding_with_trapdoor / set_simulation_key, Equation::simulate and Statement::simulate
// (include/gs_amd.hpp) on the GPU through the C ABI: proofs made WITHOUT a witness from the hiding CRS's trapdoor verify
// for random constants and random targets, are bound to their statement, rerandomize like honest ones, and are refused
// without the trapdoor, with a wrong one, on a binding CRS and for a PairingProduct equation.
// Input: the case blob of tests/test_gpu_cpp_host.py (u32 curve, type, m, n; then length-prefixed (u64) sections
//   u0 u1 v0 v1 g1 g2 gt ...; only the generators g1, g2 are used).
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

template <class FN> static bool refused(FN fn) {
  try {
    fn();
  } catch (const Panic&) {
    return false;  // a shape panic is not a refusal
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}

static std::vector<Fr> frs(MixRng& rng, size_t n) {
  std::vector<Fr> v;
  for (size_t i = 0; i < n; i++) v.push_back(rng.fr());
  return v;
}
static Matrix<Fr> mat(MixRng& rng, size_t r, size_t c) {
  Matrix<Fr> m;
  for (size_t i = 0; i < r; i++) m.push_back(frs(rng, c));
  return m;
}
// n random multiples of the generator
static std::vector<G1Affine> pts1(const CRS& crs, MixRng& rng, size_t n) {
  Bytes k = cat(frs(rng, n)), out(n * crs.ctx->sz[2]);
  crs.ctx->chk(gs_g1_mul_batch(crs.ctx->c, n, crs.g1_gen.v.data(), 1, k.data(), out.data()));
  return split<G1Affine>(out, n);
}
static std::vector<G2Affine> pts2(const CRS& crs, MixRng& rng, size_t n) {
  Bytes k = cat(frs(rng, n)), out(n * crs.ctx->sz[3]);
  crs.ctx->chk(gs_g2_mul_batch(crs.ctx->c, n, crs.g2_gen.v.data(), 1, k.data(), out.data()));
  return split<G2Affine>(out, n);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  uint32_t hdr[4];
  f.read((char*)hdr, sizeof hdr);
  const int curve = (int)hdr[0];
  Bytes u0 = section(f), u1 = section(f), v0 = section(f), v1 = section(f), g1 = section(f), g2 = section(f);
  const G1Affine p1{g1};
  const G2Affine p2{g2};

  // the same draws: the binding CRS and the hiding one share u0, v0 and differ in u1, v1
  MixRng ra{0xC0FFEEull}, rb{0xC0FFEEull};
  CRS binding = CRS::generate_crs(p1, p2, ra, curve, 0);
  auto made = CRS::generate_hiding_with_trapdoor(p1, p2, rb, curve, 0);
  const CRS& crs = made.first;
  const SimulationKey& key = made.second;
  CHECK(ra.s == rb.s);
  CHECK(binding.u[0] == crs.u[0] && binding.v[0] == crs.v[0] && !(binding.u[1] == crs.u[1]) && !(binding.v[1] == crs.v[1]));
  CHECK(key.t1.v.size() == 32 && key.t2.v.size() == 32 && !(key.t1 == key.t2));

  MixRng rng{0x51AAull};
  const size_t m = 2, n = 3;
  // random constants and RANDOM targets: no witness exists as far as anyone here knows
  MSMEG1 e1{pts1(crs, rng, n), frs(rng, m), mat(rng, m, n), pts1(crs, rng, 1)[0]};
  MSMEG2 e2{frs(rng, 1), pts2(crs, rng, m), mat(rng, m, 1), pts2(crs, rng, 1)[0]};  // over (xs[2], yg[1])
  QuadEqu e3{frs(rng, n), frs(rng, m), mat(rng, m, n), rng.fr()};
  PPE e0{pts1(crs, rng, 1), pts2(crs, rng, 1), mat(rng, 1, 1), crs.gt_gen};

  CHECK(refused([&] { e1.simulate(crs, rng); }));  // no trapdoor installed yet
  crs.set_simulation_key(key);
  CProof s1 = e1.simulate(crs, rng);
  CProof s2 = e2.simulate(crs, rng);
  CProof s3 = e3.simulate(crs, rng);
  CHECK(e1.verify(s1, crs) && e2.verify(s2, crs) && e3.verify(s3, crs));
  CHECK(s1.xcoms.coms.size() == m && s1.ycoms.coms.size() == n && s1.xcoms.rand.size() == m &&
        s1.equ_proofs[0].pi.size() == 2 && s1.equ_proofs[0].theta.size() == 1 && s1.equ_proofs[0].rand.size() == 1);
  // fresh coordinates, another proof
  CProof s1b = e1.simulate(crs, rng);
  CHECK(!(s1b.xcoms == s1.xcoms) && e1.verify(s1b, crs));
  // bound to the statement: another target is rejected
  MSMEG1 e1x = e1;
  e1x.target = pts1(crs, rng, 1)[0];
  CHECK(!e1x.verify(s1, crs));
  QuadEqu e3x = e3;
  e3x.target = rng.fr();
  CHECK(!e3x.verify(s3, crs));
  // rerandomized like any proof
  CHECK(e1.verify(e1.rerandomize(s1, crs, rng), crs));
  CHECK(e3.verify(e3.rerandomize(s3, crs, rng), crs));
  // a PairingProduct equation is refused
  CHECK(refused([&] { e0.simulate(crs, rng); }));
  // a shape mismatch is the reference's kind of panic
  {
    MSMEG1 bad = e1;
    bad.gamma.pop_back();
    bool threw = false;
    try {
      bad.simulate(crs, rng);
    } catch (const Panic&) {
      threw = true;
    }
    CHECK(threw);
  }

  // a statement of three types over shared groups xg[2], yg[1], xs[2], ys[3]
  {
    Statement st;
    st.push(e1);
    st.push(e2);
    st.push(e3);
    MSMEG1 e1c{pts1(crs, rng, n), frs(rng, m), mat(rng, m, n), pts1(crs, rng, 1)[0]};
    st.push(e1c);
    StatementProof sp = st.simulate(crs, rng);
    CHECK(sp.com_xg.coms.size() == 2 && sp.com_yg.coms.size() == 1 && sp.com_xs.coms.size() == 2 &&
          sp.com_ys.coms.size() == 3 && sp.equ_proofs.size() == 4);
    std::vector<bool> ok = st.verify(sp, crs);
    CHECK(ok.size() == 4 && ok[0] && ok[1] && ok[2] && ok[3]);
    Statement withppe;
    withppe.push(e3);
    withppe.push(e0);
    CHECK(refused([&] { withppe.simulate(crs, rng); }));
  }

  // a wrong trapdoor is refused and leaves none behind
  CHECK(refused([&] { crs.set_simulation_key(SimulationKey{key.t2, key.t1}); }));
  CHECK(refused([&] { e3.simulate(crs, rng); }));
  crs.set_simulation_key(key);
  CHECK(e3.verify(e3.simulate(crs, rng), crs));
  crs.clear_simulation_key();
  CHECK(refused([&] { e3.simulate(crs, rng); }));
  // the binding CRS of the same scalars has no trapdoor
  CHECK(refused([&] { binding.set_simulation_key(key); }));
  CHECK(refused([&] { e3.simulate(binding, rng); }));

  (void)u0, (void)u1, (void)v0, (void)v1;
  std::printf("OK %d\n", checks);
  return 0;
}
