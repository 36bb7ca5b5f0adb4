// CPU twin for the real-form Miller lines (gs_pairing.cuh: Line / line_real / line_unit, gs_tower.cuh:
// f12_mul_by_014r / _034r): the device headers compiled for the host with -DGS_FQ28_CHECK, as tests/twin/host_twin.cpp,
// behind a small C ABI of its own.  tests/test_lines_real.py builds it TWICE -- as it is and with -DGS_LINES_GENERAL --
// and compares the two.  Test infrastructure only.
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>
#include "../../groth_sahai_rs_amd/csrc/gs_params_bls12_381.h"
#include "../../groth_sahai_rs_amd/csrc/gs_params_bn254.h"
#include "../../groth_sahai_rs_amd/csrc/gs_pairing.cuh"

namespace gs {
GS_ZERO_ONE(Bls12_381)
GS_ZERO_ONE(Bn254)
}
using namespace gs;

template <class C> struct Lines {
  typedef Fq<C> F1;
  typedef Fp2<C> F2;
  static constexpr int NB = C::N * 4;  // boundary bytes of one Fq
  static F1 ld1(const uint8_t* p) { return fq_from_boundary<C>((const uint32_t*)p); }
  static void st1(uint8_t* p, const F1& a) { fq_to_boundary<C>((uint32_t*)p, a); }
  static F2 ld2(const uint8_t* p) { return {ld1(p), ld1(p + NB)}; }
  static void st2(uint8_t* p, const F2& a) { st1(p, a.c0); st1(p + NB, a.c1); }
  static Aff<F1> ldg1(const uint8_t* p) { return {ld1(p), ld1(p + NB)}; }
  static Aff<F2> ldg2(const uint8_t* p) { return {ld2(p), ld2(p + 2 * NB)}; }

  // f * (sparse element with a real coefficient) by the real product and by the general one.
  // which = 0: f12_mul_by_014(r) with (l0, l1, l4 = r);  1: f12_mul_by_034(r) with (l0 = r, l3, l4).  a, b: Fp2; r: Fq.
  // Returns the multiply-adds the real product counted (12 L^2 per dot product).
  static long sparse(int which, const uint8_t* f, const uint8_t* a, const uint8_t* b, const uint8_t* r, uint8_t* o_real,
                     uint8_t* o_general) {
    Fp12<C> x, y;
    f12_from_boundary<C>(x, (const BFq<C>*)f);
    y = x;
    const F2 fa = ld2(a), fb = ld2(b);
    const F1 fr = ld1(r);
    const F2 wide = {fr, fq_zero<C>()};
    const long m0 = fq28_mad_counter().load();
    if (which == 0) f12_mul_by_014r(x, fa, fb, fr); else f12_mul_by_034r(x, fr, fa, fb);
    const long mads = fq28_mad_counter().load() - m0;
    if (which == 0) f12_mul_by_014(y, fa, fb, wide); else f12_mul_by_034(y, wide, fa, fb);
    f12_to_boundary<C>((BFq<C>*)o_real, x);
    f12_to_boundary<C>((BFq<C>*)o_general, y);
    return mads;
  }
  // words of a kept line: 5 L in the real form, 6 L in the general one
  static int line_dwords() { return (int)(sizeof(Line<C>) / sizeof(limb_t)); }
#if !defined(GS_LINES_GENERAL)
  // in: l0, lx, ly (3 Fp2);  out: l0', lx' (2 Fp2), ly' (Fq).  what = 0: line_real, 1: line_unit (the table form)
  static void realform(int what, const uint8_t* in, uint8_t* out) {
    GLine<C> g;
    g.l0 = ld2(in), g.lx = ld2(in + 2 * NB), g.ly = ld2(in + 4 * NB);
    const Line<C> l = what == 0 ? line_real(g) : line_unit(g);
    st2(out, l.l0);
    st2(out + 2 * NB, l.lx);
    st1(out + 4 * NB, l.ly);
  }
#else
  static void realform(int, const uint8_t*, uint8_t*) {}
#endif

  // Multi-Miller value of np pairs, finally exponentiated.  mode 0: single accumulator, 1: twin (both accumulators
  // get the same G1 arguments), 2: lane pair (two host threads, the put / get discipline of the device's exchange).
  // Pairs in `mask` read a line table of their G2 argument.  out: 2 GT values (mode 0: the first only).
  static void pairing(int np, const uint8_t* ps, const uint8_t* qs, unsigned mask, uint8_t* o, int mode) {
    constexpr int NLN = miller_line_count<C>();
    std::vector<Aff<F1>> P(np);
    std::vector<Aff<F2>> Q(np);
    std::vector<Proj2<C>> T(np + 1);
    std::vector<Line<C>> tabs((size_t)np * NLN);
    std::vector<const Line<C>*> fx(np, nullptr);
    for (int i = 0; i < np; i++) {
      P[i] = ldg1(ps + i * 2 * NB);
      Q[i] = ldg2(qs + i * 4 * NB);
      if ((mask >> i) & 1) {
        miller_line_table<C>(tabs.data() + (size_t)i * NLN, Q[i]);
        fx[i] = tabs.data() + (size_t)i * NLN;
      }
    }
    Fp12<C> f, f1, e;
    if (mode == 2) {
      std::vector<int> ord;
      for (int i = 0; i < np; i++)
        if (!((mask >> i) & 1)) ord.push_back(i);
      const int nstep = (int)ord.size();
      for (int i = 0; i < np; i++)
        if ((mask >> i) & 1) ord.push_back(i);
      std::vector<Aff<F1>> Pp(np);
      std::vector<const Line<C>*> fxp(np);
      std::vector<Aff<F2>> qo[2];
      uint32_t qok = 0;
      for (int k = 0; k < np; k++) {
        Pp[k] = P[ord[k]];
        fxp[k] = fx[ord[k]];
        if (!aff_is_inf(Q[ord[k]])) qok |= 1u << k;
        if (k < nstep) qo[k & 1].push_back(Q[ord[k]]);
      }
      for (int a = 0; a < 2; a++) {
        // (odd count: lane 1 steps a copy of the last point, never consumed -- as the kernel does)
        if (nstep > 0 && (int)qo[a].size() < (nstep + 1) / 2) qo[a].push_back(Q[ord[nstep - 1]]);
        qo[a].resize((nstep + 1) / 2 + 1);
      }
      struct Exchange {
        Line<C> slot[2];
        std::atomic<int> arrived{0}, phase{0};
        void barrier() {
          int ph = phase.load();
          if (arrived.fetch_add(1) == 1) {
            arrived.store(0);
            phase.store(ph + 1);
          } else {
            while (phase.load() == ph) std::this_thread::yield();
          }
        }
      } ex;
      struct Lane {
        Exchange* ex;
        int lane;
        void put(const Line<C>& m) {
          ex->barrier();  // the partner has taken the previous line
          ex->slot[lane] = m;
          ex->barrier();
        }
        Line<C> get() const { return ex->slot[lane ^ 1]; }
      };
      Fp12<C> acc[2];
      std::thread th[2];
      for (int a = 0; a < 2; a++)
        th[a] = std::thread([&, a] {
          Lane x{&ex, a};
          std::vector<Proj2<C>> ts((nstep + 1) / 2 + 1);
          multi_miller_pair(acc[a], a, Pp.data(), qo[a].data(), qok, nstep, np, ts.data(), fxp.data(), x);
        });
      for (int a = 0; a < 2; a++) th[a].join();
      f = acc[0];
      f1 = acc[1];
    } else if (mode == 1) {
      std::vector<uint8_t> live(np);
      multi_miller2(f, f1, P.data(), P.data(), Q.data(), np, T.data(), live.data(), fx.data());
    } else {
      bool* live = new bool[np];
      multi_miller(f, P.data(), Q.data(), np, T.data(), live, fx.data());
      delete[] live;
    }
    final_exp(e, f);
    f12_to_boundary<C>((BFq<C>*)o, e);
    if (mode) {
      final_exp(e, f1);
      f12_to_boundary<C>((BFq<C>*)o + 12, e);
    }
  }
};

#define EXPORT(SUF, CURVE)                                                                                           \
  extern "C" {                                                                                                       \
  long lines_sparse_##SUF(int which, const uint8_t* f, const uint8_t* a, const uint8_t* b, const uint8_t* r,          \
                          uint8_t* o_real, uint8_t* o_general) {                                                     \
    return Lines<CURVE>::sparse(which, f, a, b, r, o_real, o_general);                                                \
  }                                                                                                                  \
  int lines_dwords_##SUF() { return Lines<CURVE>::line_dwords(); }                                                   \
  int lines_limbs_##SUF() { return CURVE::L; }                                                                       \
  void lines_realform_##SUF(int what, const uint8_t* in, uint8_t* out) { Lines<CURVE>::realform(what, in, out); }    \
  void lines_pairing_##SUF(int np, const uint8_t* ps, const uint8_t* qs, unsigned mask, uint8_t* o, int mode) {       \
    Lines<CURVE>::pairing(np, ps, qs, mask, o, mode);                                                                 \
  }                                                                                                                  \
  }
EXPORT(bls12_381, Bls12_381)
EXPORT(bn254, Bn254)
