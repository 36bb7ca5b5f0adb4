// Equation::evaluate / is_satisfied_by and Statement::evaluate / is_satisfied_by (include/gs_amd.hpp) on the GPU through
// the C ABI, on a recorded case of any of the four types: the value at the recorded witness IS the recorded target, the
// witness satisfies the equation, a changed constant or a changed target does not, a one-equation-per-call Statement
// agrees with the equations taken alone, and shape errors panic before the ABI is crossed.
// Input: the case blob of tests/test_gpu_cpp_host.py (u32 curve, type, m, n; then length-prefixed (u64) sections
//   u0 u1 v0 v1 g1 g2 gt X Y A B Gamma target ...; the sections after the target are not read).
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

template <class FN> static bool panics(FN fn) {
  try {
    fn();
  } catch (const Panic&) {
    return true;
  }
  return false;
}

// the variables of one equation as the group of a StatementVars it is over
static void put(StatementVars& v, const std::vector<G1Affine>& x) { v.xg = x; }
static void put(StatementVars& v, const std::vector<G2Affine>& y) { v.yg = y; }
static void put_x(StatementVars& v, const std::vector<Fr>& x) { v.xs = x; }
static void put_x(StatementVars& v, const std::vector<G1Affine>& x) { put(v, x); }
static void put_y(StatementVars& v, const std::vector<Fr>& y) { v.ys = y; }
static void put_y(StatementVars& v, const std::vector<G2Affine>& y) { put(v, y); }

template <class A1, class A2, class AT, EquType TY>
static void run(const CRS& crs, uint32_t m, uint32_t n, const Bytes& X, const Bytes& Y, const Bytes& A, const Bytes& B,
                const Bytes& G, const Bytes& tgt) {
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

  // the value at the recorded witness is the recorded target, byte for byte
  AT value = equ.evaluate(xvars, yvars, crs);
  CHECK(value.v == tgt);
  CHECK(equ.is_satisfied_by(xvars, yvars, crs));

  // another Gamma_00: another value, and the witness no longer satisfies the equation with the old target
  Equ other = equ;
  other.gamma[0][0] = gflat[0].v == Bytes(gflat[0].v.size(), 0) ? gflat[m * n - 1] : Fr{Bytes(gflat[0].v.size(), 0)};
  AT value2 = other.evaluate(xvars, yvars, crs);
  if (!(other.gamma[0][0] == equ.gamma[0][0])) {
    CHECK(value2.v != tgt);
    CHECK(!other.is_satisfied_by(xvars, yvars, crs));
    other.target = value2;  // ... but it does with its own value as the target
    CHECK(other.is_satisfied_by(xvars, yvars, crs));
  }
  // a target with a flipped bit is another element (or no element at all): never satisfied
  Equ wrong = equ;
  wrong.target.v[3] ^= 0x10;
  CHECK(!wrong.is_satisfied_by(xvars, yvars, crs));

  // a Statement of three equations over the shared variables: the recorded one, the changed one, the wrong-target one
  Statement st;
  st.push(equ);
  st.push(other);
  st.push(wrong);
  StatementVars vars;
  put_x(vars, xvars);
  put_y(vars, yvars);
  std::vector<Bytes> vals = st.evaluate(vars, crs);
  CHECK(vals.size() == 3);
  CHECK(vals[0] == tgt && vals[1] == value2.v && vals[2] == tgt);
  std::vector<bool> sat = st.is_satisfied_by(vars, crs);
  CHECK(sat.size() == 3);
  CHECK(sat[0] && sat[1] && !sat[2]);

  // shapes: what the reference's asserts would catch is a Panic here, before the ABI is crossed
  {
    auto fewer = xvars;
    fewer.pop_back();
    CHECK(panics([&] { equ.evaluate(fewer, yvars, crs); }));
    CHECK(panics([&] { equ.is_satisfied_by(fewer, yvars, crs); }));
    CHECK(panics([&] { equ.evaluate(std::vector<A1>{}, yvars, crs); }));
    Equ ragged = equ;
    ragged.gamma[0].pop_back();
    CHECK(panics([&] { ragged.evaluate(xvars, yvars, crs); }));
    Equ short_target = equ;
    short_target.target.v.pop_back();
    CHECK(panics([&] { short_target.is_satisfied_by(xvars, yvars, crs); }));
    StatementVars none;
    CHECK(panics([&] { st.evaluate(none, crs); }));
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  uint32_t hdr[4];
  f.read((char*)hdr, 16);
  if (!f) return 2;
  uint32_t curve = hdr[0], ty = hdr[1], m = hdr[2], n = hdr[3];
  Bytes u0 = section(f), u1 = section(f), v0 = section(f), v1 = section(f), g1 = section(f), g2 = section(f),
        gt = section(f);
  Bytes X = section(f), Y = section(f), A = section(f), B = section(f), G = section(f), tgt = section(f);
  CRS crs({Com1{u0}, Com1{u1}}, {Com2{v0}, Com2{v1}}, G1Affine{g1}, G2Affine{g2}, GT{gt}, (int)curve);
  switch (ty) {
    case 0: run<G1Affine, G2Affine, GT, EquType::PairingProduct>(crs, m, n, X, Y, A, B, G, tgt); break;
    case 1: run<G1Affine, Fr, G1Affine, EquType::MultiScalarG1>(crs, m, n, X, Y, A, B, G, tgt); break;
    case 2: run<Fr, G2Affine, G2Affine, EquType::MultiScalarG2>(crs, m, n, X, Y, A, B, G, tgt); break;
    case 3: run<Fr, Fr, Fr, EquType::Quadratic>(crs, m, n, X, Y, A, B, G, tgt); break;
    default: return 2;
  }
  std::printf("OK %d\n", checks);
  return 0;
}
