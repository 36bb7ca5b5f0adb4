// One table of arithmetic operations on RAW internal limb vectors, shared by the device probe (arith_probe.hip) and the
// CPU twin (tests/twin/host_twin.cpp, twin_raw_op_<curve>): the operand sets of tests/arithvec.py go through the same
// dispatch in both.  Test infrastructure only.  Include after gs_pairing.cuh, at file scope.
//
// An item is NIN base-field operands of C::L int32 limbs each and gives NOUT results of C::L int32 each (tests/arithvec.py,
// OPS, holds the same shapes).  Flags are returned in limb 0 of a result; boundary words (C::N u32) travel in the first
// C::N limbs of a slot.  Operands outside an operation's contract are never sent here.
namespace arith {
using namespace gs;

template <class C> GS_HD Fq<C> ldq(const int32_t* p) {
  Fq<C> r;
  for (int i = 0; i < C::L; i++) r.v[i] = p[i];
  return r;
}
template <class C> GS_HD void stq(int32_t* p, const Fq<C>& a) {
  for (int i = 0; i < C::L; i++) {
#if defined(GS_FQ28_CHECK)
    if (a.v[i] >= ((int64_t)1 << 31) || a.v[i] < -((int64_t)1 << 31)) {
      fprintf(stderr, "raw op: a result limb leaves int32\n");
      abort();
    }
#endif
    p[i] = (int32_t)a.v[i];
  }
}
template <class C> GS_HD void stflag(int32_t* p, bool f) {
  for (int i = 0; i < C::L; i++) p[i] = 0;
  p[0] = f ? 1 : 0;
}
template <class C> GS_HD Fp2<C> ld2(const int32_t* p) { return {ldq<C>(p), ldq<C>(p + C::L)}; }
template <class C> GS_HD void st2(int32_t* p, const Fp2<C>& a) {
  stq<C>(p, a.c0);
  stq<C>(p + C::L, a.c1);
}
template <class C> GS_HD void ld6(Fp6<C>& r, const int32_t* p) {
  r.c0 = ld2<C>(p);
  r.c1 = ld2<C>(p + 2 * C::L);
  r.c2 = ld2<C>(p + 4 * C::L);
}
template <class C> GS_HD void st6(int32_t* p, const Fp6<C>& a) {
  st2<C>(p, a.c0);
  st2<C>(p + 2 * C::L, a.c1);
  st2<C>(p + 4 * C::L, a.c2);
}
template <class C> GS_HD void ld12(Fp12<C>& r, const int32_t* p) {
  ld6<C>(r.c0, p);
  ld6<C>(r.c1, p + 6 * C::L);
}
template <class C> GS_HD void st12(int32_t* p, const Fp12<C>& a) {
  st6<C>(p, a.c0);
  st6<C>(p + 6 * C::L, a.c1);
}

enum Op {
  FQ_MUL = 0, FQ_SQR, FQ_NORM, FQ_NORM_FULL, FQ_VREDUCE, FQ_IS_ZERO, FQ_IS_ZERO_SLOW, FQ_EQ, FQ_INV, FQ_FROM_BOUNDARY,
  FQ_TO_BOUNDARY, F2_MUL, F2_MUL_L2, F2_SQR, F2_SQR_L2, F2_DOT3, F2_MUL_XI, F2_MUL_FP, F2_INV, F6_MUL, F6_MUL_BY_01,
  F12_MUL, F12_SQR, F12_MUL_BY_014, F12_MUL_BY_034, F12_CYCLO_CHAIN, F12_INV, F12_FROB, F12_EQ, G1_DBL, G1_MADD, G1_ADD,
  G2_DBL, G2_MADD, G2_ADD, F12_CYCLO_SQR, NUM_OPS
};
// the base-field and Fp2 families (all that the probe's second build, the one with the inline multiplier forms, compiles)
#define ARITH_FOR_EACH_BASE_FP2_OP(X) \
  X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18)
#if defined(ARITH_BASE_FP2_ONLY)
#define ARITH_FOR_EACH_OP(X) ARITH_FOR_EACH_BASE_FP2_OP(X)
#else
#define ARITH_FOR_EACH_OP(X)                                                                                 \
  ARITH_FOR_EACH_BASE_FP2_OP(X)                                                                              \
  X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32) X(33) X(34) X(35)
#endif

// operands in, results out, in units of one base-field element
constexpr int op_nin(int op) {
  constexpr int t[NUM_OPS] = {2, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 4, 4, 2, 2, 12, 2, 3, 2, 12, 10, 24, 12, 18, 18, 12, 12, 12, 24,
                              3, 5, 6, 6, 10, 12, 12};
  return t[op];
}
constexpr int op_nout(int op) {
  constexpr int t[NUM_OPS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 6, 6, 12, 12, 12, 12, 12, 12, 36, 1,
                              3, 3, 3, 6, 6, 6, 12};
  return t[op];
}
constexpr int CYCLO_STEPS = 9;  // cyclotomic squarings of F12_CYCLO_CHAIN, a value reduction after every third (the x-power loop)

template <class C, int OP> GS_HD void arith_op(const int32_t* in, int32_t* out) {
  constexpr int L = C::L;
  if constexpr (OP == FQ_MUL) {
    stq<C>(out, mul(ldq<C>(in), ldq<C>(in + L)));
  } else if constexpr (OP == FQ_SQR) {
    stq<C>(out, sqr(ldq<C>(in)));
  } else if constexpr (OP == FQ_NORM) {
    stq<C>(out, norm(ldq<C>(in)));
  } else if constexpr (OP == FQ_NORM_FULL) {
    stq<C>(out, norm_full(ldq<C>(in)));
  } else if constexpr (OP == FQ_VREDUCE) {
    stq<C>(out, vreduce(ldq<C>(in)));
  } else if constexpr (OP == FQ_IS_ZERO) {
    stflag<C>(out, is_zero(ldq<C>(in)));
  } else if constexpr (OP == FQ_IS_ZERO_SLOW) {
    stflag<C>(out, is_zero_slow(ldq<C>(in)));
  } else if constexpr (OP == FQ_EQ) {
    stflag<C>(out, eq(ldq<C>(in), ldq<C>(in + L)));
  } else if constexpr (OP == FQ_INV) {
    stq<C>(out, inv(ldq<C>(in)));
  } else if constexpr (OP == FQ_FROM_BOUNDARY) {
    uint32_t w[C::N];
    for (int i = 0; i < C::N; i++) w[i] = (uint32_t)in[i];
    stq<C>(out, fq_from_boundary<C>(w));
  } else if constexpr (OP == FQ_TO_BOUNDARY) {
    uint32_t w[C::N];
    fq_to_boundary<C>(w, ldq<C>(in));
    for (int i = 0; i < L; i++) out[i] = i < C::N ? (int32_t)w[i] : 0;
  } else if constexpr (OP == F2_MUL) {
    st2<C>(out, mul(ld2<C>(in), ld2<C>(in + 2 * L)));
  } else if constexpr (OP == F2_MUL_L2) {
    st2<C>(out, mul_l2(ld2<C>(in), ld2<C>(in + 2 * L)));
  } else if constexpr (OP == F2_SQR) {
    st2<C>(out, sqr(ld2<C>(in)));
  } else if constexpr (OP == F2_SQR_L2) {
    st2<C>(out, sqr_l2(ld2<C>(in)));
  } else if constexpr (OP == F2_DOT3) {
    st2<C>(out, dot3(ld2<C>(in), ld2<C>(in + 2 * L), ld2<C>(in + 4 * L), ld2<C>(in + 6 * L), ld2<C>(in + 8 * L),
                     ld2<C>(in + 10 * L)));
  } else if constexpr (OP == F2_MUL_XI) {
    st2<C>(out, mul_xi(ld2<C>(in)));
  } else if constexpr (OP == F2_MUL_FP) {
    st2<C>(out, mul_fp(ld2<C>(in), ldq<C>(in + 2 * L)));
  } else if constexpr (OP == F2_INV) {
    st2<C>(out, inv(ld2<C>(in)));
  } else if constexpr (OP == F6_MUL) {
    Fp6<C> a, b, r;
    ld6<C>(a, in);
    ld6<C>(b, in + 6 * L);
    f6_mul(r, a, b);
    st6<C>(out, r);
  } else if constexpr (OP == F6_MUL_BY_01) {
    Fp6<C> a, r;
    ld6<C>(a, in);
    f6_mul_by_01(r, a, ld2<C>(in + 6 * L), ld2<C>(in + 8 * L));
    st6<C>(out, r);
  } else if constexpr (OP == F12_MUL) {
    Fp12<C> a, b, r;
    ld12<C>(a, in);
    ld12<C>(b, in + 12 * L);
    f12_mul(r, a, b);
    st12<C>(out, r);
  } else if constexpr (OP == F12_SQR) {
    Fp12<C> a, r;
    ld12<C>(a, in);
    f12_sqr(r, a);
    st12<C>(out, r);
  } else if constexpr (OP == F12_MUL_BY_014 || OP == F12_MUL_BY_034) {
    Fp12<C> f;
    ld12<C>(f, in);
    if constexpr (OP == F12_MUL_BY_014)
      f12_mul_by_014(f, ld2<C>(in + 12 * L), ld2<C>(in + 14 * L), ld2<C>(in + 16 * L));
    else
      f12_mul_by_034(f, ld2<C>(in + 12 * L), ld2<C>(in + 14 * L), ld2<C>(in + 16 * L));
    st12<C>(out, f);
  } else if constexpr (OP == F12_CYCLO_CHAIN) {
    Fp12<C> f, t;
    ld12<C>(f, in);
    for (int i = 1; i <= CYCLO_STEPS; i++) {
      f12_cyclo_sqr(t, f);
      f = t;
      if (i % 3 == 0) f12_vreduce(f);
    }
    st12<C>(out, f);
  } else if constexpr (OP == F12_CYCLO_SQR) {
    // ONE Granger-Scott squaring: its formulas are polynomial, so they are checked on arbitrary (extreme) coefficients too
    Fp12<C> f, t;
    ld12<C>(f, in);
    f12_cyclo_sqr(t, f);
    st12<C>(out, t);
  } else if constexpr (OP == F12_INV) {
    Fp12<C> a, r;
    ld12<C>(a, in);
    f12_inv(r, a);
    st12<C>(out, r);
  } else if constexpr (OP == F12_FROB) {
    Fp12<C> a, r;
    ld12<C>(a, in);
    for (int j = 1; j <= 3; j++) {
      f12_frob(r, a, j);
      st12<C>(out + (j - 1) * 12 * L, r);
    }
  } else if constexpr (OP == F12_EQ) {
    Fp12<C> a, b;
    ld12<C>(a, in);
    ld12<C>(b, in + 12 * L);
    stflag<C>(out, f12_eq(a, b));
  } else if constexpr (OP == G1_DBL || OP == G1_MADD || OP == G1_ADD) {
    // the entry points the scalar-multiplication loops use: on the device the generated subroutines, their edge cases in C++
    Jac<Fq<C>> r = {ldq<C>(in), ldq<C>(in + L), ldq<C>(in + 2 * L)};
    if constexpr (OP == G1_DBL) {
      jac_dbl_ip(r);
    } else if constexpr (OP == G1_MADD) {
      Aff<Fq<C>> q = {ldq<C>(in + 3 * L), ldq<C>(in + 4 * L)};
      jac_madd_ip(r, q);
    } else {
      Jac<Fq<C>> q = {ldq<C>(in + 3 * L), ldq<C>(in + 4 * L), ldq<C>(in + 5 * L)}, s;
      jac_add(s, r, q);
      r = s;
    }
    stq<C>(out, r.x);
    stq<C>(out + L, r.y);
    stq<C>(out + 2 * L, r.z);
  } else {
    static_assert(OP == G2_DBL || OP == G2_MADD || OP == G2_ADD, "unknown operation");
    Jac<Fp2<C>> r = {ld2<C>(in), ld2<C>(in + 2 * L), ld2<C>(in + 4 * L)};
    if constexpr (OP == G2_DBL) {
      jac_dbl_ip(r);
    } else if constexpr (OP == G2_MADD) {
      Aff<Fp2<C>> q = {ld2<C>(in + 6 * L), ld2<C>(in + 8 * L)};
      jac_madd_ip(r, q);
    } else {
      Jac<Fp2<C>> q = {ld2<C>(in + 6 * L), ld2<C>(in + 8 * L), ld2<C>(in + 10 * L)}, s;
      jac_add(s, r, q);
      r = s;
    }
    st2<C>(out, r.x);
    st2<C>(out + 2 * L, r.y);
    st2<C>(out + 4 * L, r.z);
  }
}

}  // namespace arith
