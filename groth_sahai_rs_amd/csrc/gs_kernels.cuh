// Device kernels of the Groth-Sahai engine.  One lane = one task; a task is a
// descriptor-driven unit of group arithmetic, so that the four equation types
// of the reference (src/statement.rs:117-192) and both groups share the same
// handful of kernels.  Per batch the host (gs_amd.hip) uploads small per-shape
// task tables; per-equation data is addressed as  base[arr] + eq*stride[arr].
//
//   k_prep_*   Fr mini-GEMMs  Psi = R^T Gamma, Omega = Psi S - T^T, Phi = S^T Gamma^T
//              (prove.rs:133,139-142,154) -> canonical scalars in the "pool"
//   k_var      one variable-base scalar multiplication per lane (Jacobian out)
//   k_fix      <= 2 fixed-base terms from the CRS window tables (+ affine addend)
//   k_red      sum the partial slots of a commitment-group element, ONE shared
//              inversion per element (Montgomery trick), normalised affine out
//   k_miller   multi-Miller loop over <= 3 pairs  -> un-exponentiated Fp12
//   k_final    product of a cell's partial Miller values, final exponentiation,
//              compare (verifier.rs:50-53)
#pragma once
#include <type_traits>
#include <utility>

#include "gs_pairing.cuh"
#include "gs_coop.cuh"
#include "gs_wire.cuh"

namespace gs {

#ifndef GS_WPE
#define GS_WPE 1
#endif
constexpr int MAX_ARR = 8;
struct ArrTab {
  const uint8_t* base[MAX_ARR];
  uint32_t stride[MAX_ARR];  // bytes per equation; 0 = shared by the whole batch
};
struct OutTab {
  uint8_t* base[4];
  uint32_t stride[4];
};
struct VarTask {
  uint32_t s_idx, p_idx, slot;  // 32-bit: large-arity equations (m, n ~ 334, benches/bench.rs:451-498) have > 2^16 scalars
  uint8_t p_arr, neg, pad0, pad1;  // neg: use -P
};
constexpr int GRP_OUT = 4;  // outputs one Straus lane can serve from one table build
struct GrpTask {  // one lane of k_var_multi: `no` outputs over the SAME nt bases (in the same order, same signs);
  uint32_t nt, no;             // output o sums VarTasks first[o] .. first[o] + nt - 1 into slot[o]
  uint32_t first[GRP_OUT], slot[GRP_OUT];
};
struct FixTask {
  uint32_t s0, s1, a_idx, slot;
  uint8_t t0, t1, a_arr, a_neg;  // 0xFF = absent
};
struct RedTask {
  uint32_t b0, e0, b1, e1, out_idx;
  uint8_t out_arr, pad, pad1, pad2;
};
// one G2 argument with its TWO G1 partners: P(a) = parr[p_arr][p_idx + a], a = 0, 1
struct PairRef {
  uint8_t p_arr, q_arr, neg, pad;
  uint32_t p_idx, q_idx;
};
#ifndef GS_MILLER_CAP
#define GS_MILLER_CAP 12
#endif
constexpr int MILLER_CH = GS_MILLER_CAP;  // capacity of a Miller lane; the host picks the chunk per batch size
struct MillerTask {
  uint8_t np, b, single, pad1;  // single: only the P(0) partner is used (one accumulator)
  PairRef pr[MILLER_CH];
};
// where the Miller partials of cell c = 2a + b live: tasks [lo, hi), slot sub (0/1) of each task
struct CellMap {
  int lo[4], hi[4], sub[4];
};
struct PoolMap {  // offsets (in scalars) into the per-equation pool
  int RC, SC, PSI, PHI, OM, TC, RHO, SIG, XC, YC, GC, AC, BC, NT, RH, AR, NR, total;
};

template <class T> __device__ __forceinline__ T ld(const uint8_t* p) { return *reinterpret_cast<const T*>(p); }

// ---- segmented launches ---------------------------------------------------------------------------------------------
// The kernels of the prove / verify path are written as BODIES: `struct k_xxx { static __device__ void run(size_t g,
// args...); }`, g = the lane's index within its launch.  One generic __global__ function, k_seg<Body, args...>, runs a
// body over up to MAX_SEG SEGMENTS: consecutive, block-aligned lane ranges with their own argument packs.  An ordinary
// launch is one segment.  A mixed batch (gs_prove_mixed / gs_verify_mixed: sub-batches of different equation types and
// shapes, each with its own task tables and arrays) MERGES the launches of its parts that run the same body into one
// launch with a segment per part, so that a few thousand equations of three types fill the chip like a homogeneous
// batch of their total size -- dispatches from several streams do not share these 512-register kernels' SIMDs
// (profiles/r3/mixed_streams.txt).  The segment of a lane is wave-uniform (segments start at block boundaries, blocks
// are one wave), so its argument pack is read with scalar loads from the kernel-argument segment exactly as the
// arguments of an ordinary kernel are.
constexpr int MAX_SEG = 4;
template <size_t I, class T> struct PackLeaf {
  T v;
};
template <class Seq, class... A> struct PackImpl;
template <size_t... I, class... A> struct PackImpl<std::index_sequence<I...>, A...> : PackLeaf<I, A>... {};
template <class... A> using Pack = PackImpl<std::index_sequence_for<A...>, A...>;
template <size_t I, class T> __host__ __device__ __forceinline__ const T& pack_get(const PackLeaf<I, T>& l) { return l.v; }
template <class... A> struct Segs {
  int n, pad;
  // clock stamps (kernel profile only, else null): every wave adds its own d s_memtime (shader cycles), d s_memrealtime
  // (100 MHz) and 1 to stamp[0..2], so that the host reads the clock THIS launch ran at -- sum d memtime / sum d
  // memrealtime x 100 MHz -- from the launch it has just timed (bench.py: the ALU peak at the kernel's own clock)
  unsigned long long* stamp;
  size_t lo[MAX_SEG];  // first lane of each segment (multiples of the block size, ascending; lo[0] = 0)
  Pack<A...> a[MAX_SEG];
};
template <class Body, class... A, size_t... I>
__device__ __forceinline__ void seg_call(size_t g, const Pack<A...>& p, std::index_sequence<I...>) {
  Body::run(g, pack_get<I>(p)...);
}
#ifndef GS_KSEG_ATTR
#define GS_KSEG_ATTR
#endif
// waves per SIMD a body is BUILT for (the second argument of __launch_bounds__ = the minimum the compiler must allow:
// 2 caps the kernel at 256 registers).  Default 1: every heavy kernel owns the whole register file of its SIMD.
template <class B, class = void> struct BodyWpe {
  static constexpr int v = GS_WPE;
};
template <class B> struct BodyWpe<B, std::void_t<decltype(B::WPE)>> {
  static constexpr int v = B::WPE;
};
template <class Body, class... A> __global__ void __launch_bounds__(64, BodyWpe<Body>::v) GS_KSEG_ATTR k_seg(Segs<A...> S) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  int s = 0;
  for (int i = 1; i < S.n; i++)
    if (g >= S.lo[i]) s = i;
  s = __builtin_amdgcn_readfirstlane(s);
  unsigned long long t0 = 0, r0 = 0;
  if (S.stamp) {
    t0 = __builtin_amdgcn_s_memtime();
    r0 = __builtin_amdgcn_s_memrealtime();
  }
  seg_call<Body>(g - S.lo[s], S.a[s], std::index_sequence_for<A...>{});
  if (S.stamp) {  // (a body's early `return` ends the inlined body, not the kernel: every wave gets here)
    unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
      atomicAdd(S.stamp, t1 - t0);
      atomicAdd(S.stamp + 1, r1 - r0);
      atomicAdd(S.stamp + 2, 1ull);
    }
  }
}

// ---- boundary <-> internal I/O --------------------------------------------------
// API arrays hold arkworks' saturated Montgomery limbs (BFq); everything the
// kernels keep between launches (window tables, Jacobian partials, Miller partials)
// stays in the internal radix-2^28 form.
template <class C> constexpr size_t aff_bytes(const Aff<Fq<C>>*) { return 2 * sizeof(BFq<C>); }
template <class C> constexpr size_t aff_bytes(const Aff<Fp2<C>>*) { return 4 * sizeof(BFq<C>); }
template <class C> GS_HD void aff_load(Aff<Fq<C>>& r, const uint8_t* p) {
  const BFq<C>* b = reinterpret_cast<const BFq<C>*>(p);
  BFq<C> x = b[0], y = b[1];
  r.x = fq_from_boundary<C>(x.w);
  r.y = fq_from_boundary<C>(y.w);
}
template <class C> GS_HD void aff_load(Aff<Fp2<C>>& r, const uint8_t* p) {
  const BFq<C>* b = reinterpret_cast<const BFq<C>*>(p);
  BFq<C> t[4] = {b[0], b[1], b[2], b[3]};
  r.x = fp2_from_boundary<C>(t);
  r.y = fp2_from_boundary<C>(t + 2);
}
template <class C> GS_HD void aff_store(uint8_t* p, const Aff<Fq<C>>& a) {
  BFq<C>* b = reinterpret_cast<BFq<C>*>(p);
  BFq<C> x, y;
  fq_to_boundary<C>(x.w, a.x);
  fq_to_boundary<C>(y.w, a.y);
  b[0] = x;
  b[1] = y;
}
template <class C> GS_HD void aff_store(uint8_t* p, const Aff<Fp2<C>>& a) {
  BFq<C>* b = reinterpret_cast<BFq<C>*>(p);
  BFq<C> t[4];
  fp2_to_boundary<C>(t, a.x);
  fp2_to_boundary<C>(t + 2, a.y);
  b[0] = t[0];
  b[1] = t[1];
  b[2] = t[2];
  b[3] = t[3];
}
#define AFFB(C, F) (aff_bytes<C>((const Aff<F>*)nullptr))

// --------------------------------------------------------------------------
// generic helpers
// --------------------------------------------------------------------------
template <class C, class F, bool ENDO = true>
__global__ void __launch_bounds__(64, GS_WPE) k_smul_batch(size_t n, const uint8_t* p, int broadcast, const Fr<C>* k,
                                                   uint8_t* out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Aff<F> P;
  aff_load<C>(P, p + (broadcast ? 0 : i) * AFFB(C, F));
  Jac<F> J;
  jac_smul_any<C, F, ENDO>(J, P, from_mont(k[i]));
  Aff<F> R;
  jac_to_aff(R, J);
  aff_store<C>(out + i * AFFB(C, F), R);
}

// pts[5] <- pts[3] + pts[5]  (W.1 = u1.1 + generator), single lane
template <class C, class F> __global__ void k_crs_derive(uint8_t* pts) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Aff<F> a, b;
  aff_load<C>(a, pts + 3 * AFFB(C, F));
  aff_load<C>(b, pts + 5 * AFFB(C, F));
  Jac<F> j;
  jac_from_aff(j, a);
  jac_madd(j, j, b);
  Aff<F> r;
  jac_to_aff(r, j);
  aff_store<C>(pts + 5 * AFFB(C, F), r);
}

// ---- witness extraction with the binding key (gs_extract_*) -----------------------------------------------------------
// The CRS of gs_crs_generate has u0 = (p, a p), u1 = t u0, so a commitment c = (O, X) + r0 u0 + r1 u1 opens to
// X = c.1 - a c.0 for whoever holds a.  out[i] = coms[i].1 - a coms[i].0, one lane per commitment, `a` the same in every
// lane: its digit streams are made once at key-set time (k_extract_key) and read here through the scalar path
// (jac_smul_shared).  The subtraction is one more addition on the running point: a c.0 + (-c.1), negated -- the mixed
// addition's own edge cases cover a c.0 = O, c.1 = O, a c.0 = c.1 (identity out) and a c.0 = -c.1 (doubling).
template <class C, class F, bool ENDO = true>
struct k_extract {
  static __device__ __forceinline__ void run(size_t g, size_t total, const uint8_t* coms, const SharedDigits* sd,
                                            uint8_t* out) {
  if (g >= total) return;
  Aff<F> c0, c1;
  aff_load<C>(c0, coms + (2 * g) * AFFB(C, F));
  aff_load<C>(c1, coms + (2 * g + 1) * AFFB(C, F));
  Jac<F> J;
  jac_smul_shared<C, F, ENDO>(J, c0, sd);
  c1.y = neg(c1.y);  // (the identity (0, 0) stays exactly (0, 0))
  jac_madd(J, J, c1);
  J.y = neg(J.y);
  Aff<F> R;
  jac_to_aff(R, J);
  aff_store<C>(out + g * AFFB(C, F), R);
}
};

// Key-set time, lanes 0 and 1: does pts[2 i + 1] == key * pts[2 i] hold for the CRS pair i (u0, u1 or v0, v1)?  Plain
// double-and-add, so the answer is defined whatever the CRS holds.  Lane 0 also writes the key's digit streams for the
// endomorphism kernels (sd[0]) and the plain ones (sd[1]).  key: one Montgomery Fr.
template <class C, class F>
__global__ void __launch_bounds__(64, GS_WPE) k_extract_key(const Fr<C>* key, const uint8_t* pts, SharedDigits* sd,
                                                            uint8_t* ok) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= 2) return;
  const Fr<C> k = from_mont(key[0]);
  Aff<F> P, R;
  aff_load<C>(P, pts + (2 * i) * AFFB(C, F));
  Jac<F> J;
  jac_smul(J, P, k);
  jac_to_aff(R, J);
  BFq<C> got[AFFB(C, F) / sizeof(BFq<C>)];
  aff_store<C>(reinterpret_cast<uint8_t*>(got), R);
  const uint8_t *a = reinterpret_cast<const uint8_t*>(got), *b = pts + (2 * i + 1) * AFFB(C, F);
  bool same = true;
  for (size_t j = 0; j < AFFB(C, F); j++) same = same && a[j] == b[j];
  ok[i] = same ? 1 : 0;
  if (i == 0) {
    SharedDigits d;
    shared_digits<C, F, true>(d, k);
    sd[0] = d;
    shared_digits<C, F, false>(d, k);
    sd[1] = d;
  }
}

// ---- proof simulation with the hiding CRS's trapdoor (gs_simulate_*) ---------------------------------------------------
// On the CRS of gs_crs_generate_hiding W = key[1] + (O, generator) = t key[0]: whoever holds t1, t2 answers every
// equation with commitments and proofs that are fixed-base combinations of u / v, plus one short variable-base sum.
//
// Key-set time, lanes 0 and 1: does W.i == key * key0.i hold (pts = u0.0 u0.1 u1.0 u1.1 W.0 W.1, the CRS's device
// copy)?  Plain double-and-add, so the answer is defined whatever the CRS holds.  key: one Montgomery Fr.
template <class C, class F>
__global__ void __launch_bounds__(64, GS_WPE) k_sim_key(const Fr<C>* key, const uint8_t* pts, uint8_t* ok) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= 2) return;
  const Fr<C> k = from_mont(key[0]);
  Aff<F> P, R;
  aff_load<C>(P, pts + i * AFFB(C, F));
  Jac<F> J;
  jac_smul(J, P, k);
  jac_to_aff(R, J);
  BFq<C> got[AFFB(C, F) / sizeof(BFq<C>)];
  aff_store<C>(reinterpret_cast<uint8_t*>(got), R);
  const uint8_t *a = reinterpret_cast<const uint8_t*>(got), *b = pts + (4 + i) * AFFB(C, F);
  bool same = true;
  for (size_t j = 0; j < AFFB(C, F); j++) same = same && a[j] == b[j];
  ok[i] = same ? 1 : 0;
}

// one Fr that every lane of the launch reads alike (the trapdoor): through the constant address space, i.e. scalar
// loads into scalar registers, not one vector load per lane
template <class C> __device__ __forceinline__ Fr<C> ld_uniform_fr(const Fr<C>* p) {
  typedef const __attribute__((address_space(4))) uint32_t* cptr;
  cptr w = (cptr) reinterpret_cast<const uint32_t*>(p);
  Fr<C> r;
#pragma unroll
  for (int i = 0; i < FrM<C>::N; i++) r.v[i] = w[i];
  return r;
}

// The simulator's scalars, one lane per equation (all types but PPE).  Inputs in the layouts of gs_prove_batch's R, S, T:
// Rc[m][kx], Sc[n][ky] (coordinates of the commitments in the bases u / v), Tf[ky][kx] (the free proof scalars); as / bs /
// tq: the scalar constants and target where the type has them; key = t1, t2 (Montgomery).  The pool receives, canonical:
//   RC, SC   Rc, Sc: the fixed-base scalars of the commitments, and the Straus scalars of V (Sc_j for MSMEG1, Rc_i for MSMEG2)
//   TC       Tf: the fixed-base scalars of the proof elements that are multiples of u0 / v0 alone
//   OM       MSMEG1: sum_i e_i Rc_ia - Tf[0][a], e_i = t2 b_i + sum_j Gamma_ij Sc_j   (theta's coordinates on u0, u1)
//            MSMEG2: sum_j f_j Sc_jl - Tf[l][0], f_j = t1 a_j + sum_i Rc_i Gamma_ij   (pi's coordinates on v0, v1)
//            QuadEqu: t2 sum_i Rc_i b_i + t1 sum_j a_j Sc_j + sum_ij Rc_i Gamma_ij Sc_j - t t1 t2 - Tf[0][0]   (pi = OM v0)
//   NT       -t2 (MSMEG1) / -t1 (MSMEG2): the Straus scalar of the target in V
// shared_vars: a Statement -- ONE copy of Rc, Sc for all equations.
template <class C>
struct k_prep_sim {
  static __device__ __forceinline__ void run(size_t e, size_t N, int ty, int m, int n, const Fr<C>* G, const Fr<C>* as,
                                            const Fr<C>* bs, const Fr<C>* tq, const Fr<C>* R, const Fr<C>* S,
                                            const Fr<C>* T, const Fr<C>* key, PoolMap pm, Fr<C>* pool, int shared_vars) {
  if (e >= N) return;
  typedef Fr<C> S_;
  const int kx = (ty == 1) ? 2 : 1, ky = (ty == 2) ? 2 : 1;
  const size_t ev = shared_vars ? 0 : e;
  G += e * m * n;
  R += ev * m * kx;
  S += ev * n * ky;
  T += e * ky * kx;
  const S_ t1 = ld_uniform_fr<C>(key), t2 = ld_uniform_fr<C>(key + 1);
  S_* P = pool + e * pm.total;
  for (int i = 0; i < m * kx; i++) P[pm.RC + i] = from_mont(R[i]);
  for (int i = 0; i < n * ky; i++) P[pm.SC + i] = from_mont(S[i]);
  for (int i = 0; i < ky * kx; i++) P[pm.TC + i] = from_mont(T[i]);
  S_ c0 = fzero<FrM<C>>(), c1 = fzero<FrM<C>>();
  if (ty == 1) {
    bs += e * m;
    for (int i = 0; i < m; i++) {
      S_ ei = mul(t2, bs[i]);
      for (int j = 0; j < n; j++) ei = add(ei, mul(G[i * n + j], S[j]));
      c0 = add(c0, mul(ei, R[2 * i]));
      c1 = add(c1, mul(ei, R[2 * i + 1]));
    }
    P[pm.OM] = from_mont(sub(c0, T[0]));
    P[pm.OM + 1] = from_mont(sub(c1, T[1]));
    P[pm.NT] = from_mont(neg(t2));
  } else if (ty == 2) {
    as += e * n;
    for (int j = 0; j < n; j++) {
      S_ fj = mul(t1, as[j]);
      for (int i = 0; i < m; i++) fj = add(fj, mul(R[i], G[i * n + j]));
      c0 = add(c0, mul(fj, S[2 * j]));
      c1 = add(c1, mul(fj, S[2 * j + 1]));
    }
    P[pm.OM] = from_mont(sub(c0, T[0]));
    P[pm.OM + 1] = from_mont(sub(c1, T[1]));
    P[pm.NT] = from_mont(neg(t1));
  } else {
    as += e * n;
    bs += e * m;
    for (int i = 0; i < m; i++) {
      S_ ei = mul(t2, bs[i]);
      for (int j = 0; j < n; j++) ei = add(ei, mul(G[i * n + j], S[j]));
      c0 = add(c0, mul(ei, R[i]));
    }
    for (int j = 0; j < n; j++) c1 = add(c1, mul(as[j], S[j]));
    c0 = add(c0, mul(t1, c1));
    c0 = sub(c0, mul(tq[e], mul(t1, t2)));
    P[pm.OM] = from_mont(sub(c0, T[0]));
  }
}
};

// ---- bounded discrete logarithms (gs_dlog_*, gs_extract_scalar_*) ------------------------------------------------------
// Baby-step giant-step for x in [0, 2^bits) with x G = P.  B = 2^log2_table baby steps j G,
// j = 1..B, are kept by the x coordinate alone (one entry serves +j and -j) in an open-addressing table of 2 B slots of
// 64 bits, slot = fingerprint << 29 | j, 0 = empty.  The giant steps have stride S = 2 B and centres c_t = B + t S:
// x = c_t + d, d in [-B, B), and the lane looks for the x coordinate of Q_t = P - c_t G = d G in the table.
constexpr int DLOG_JBITS = 29;                 // j <= 2^28
constexpr int DLOG_FP_BITS = 64 - DLOG_JBITS;  // fingerprint bits of a slot (the default of "dlog_fp_bits")
constexpr int DLOG_RUN = 8;                    // consecutive baby steps per lane of k_dlog_table
// LDS of a k_dlog block (one wave): a quarter of the CU's 160 KB, so that each of its four SIMDs holds a wave
constexpr int DLOG_LDS_BYTES = 40 * 1024;
constexpr int DLOG_KMAX = 16;
// giant steps per launch unless "dlog_steps" says otherwise.  An ESTIMATE, not a measured optimum: ~6 Fq
// multiplications per G1 step at ~2 10^6 multiplications per second and lane make this ~0.1 s (G2 ~0.3 s).
constexpr uint32_t DLOG_STEPS_DEFAULT = 1u << 15;
template <class F> struct DlogShape {
  static constexpr int NW = (int)(sizeof(F) / sizeof(limb_t));
  static constexpr int KFIT = DLOG_LDS_BYTES / (64 * (int)sizeof(F));
  // giant steps under one shared inversion: what fits the block's LDS share (BLS12-381: 11 in G1, 5 in G2; BN254: 16, 8)
  static constexpr int K = KFIT > DLOG_KMAX ? DLOG_KMAX : KFIT;
  static_assert(K >= 2, "giant steps per inversion");
};

// The key of a coordinate: its CANONICAL value (two lazy representations of one x must hash alike), all words mixed.
template <class C, class F> __device__ __forceinline__ uint64_t dlog_hash(const F& x) {
  uint32_t w[NCoord<F>::V][C::N];
  coord_words<C>(w, x);
  uint64_t h = 0x243F6A8885A308D3ull;
  for (int a = 0; a < NCoord<F>::V; a++)
    for (int i = 0; i < C::N; i++) {
      h = (h ^ w[a][i]) * 0x9E3779B97F4A7C15ull;
      h ^= h >> 29;
    }
  h *= 0xD6E8FEB86659FD93ull;
  return h ^ (h >> 32);
}
// r = k G for a short scalar: plain double-and-add from the top bit, full edge cases (any curve point)
template <class F> GS_HD_NOINLINE void jac_smul_u64(Jac<F>& rout, const Aff<F>& g, uint64_t k) {
  Jac<F> r;
  jac_set_inf(r);
  int top = -1;
  for (int i = 0; i < 64; i++)
    if ((k >> i) & 1) top = i;
#pragma unroll 1
  for (int i = top; i >= 0; i--) {
    jac_dbl(r, r);
    if ((k >> i) & 1) jac_madd_edge(r, r, g);
  }
  rout = r;
}
// x G == P on full coordinates (P is not the identity)
template <class C, class F> GS_HD_NOINLINE bool dlog_confirm(const Aff<F>& G, const Aff<F>& P, uint64_t x) {
  Jac<F> j;
  jac_smul_u64(j, G, x);
  if (is_zero_limbs(j.z)) return false;
  Aff<F> r;
  jac_to_aff(r, j);
  return eq(r.x, P.x) && eq(r.y, P.y);  // exact comparisons mod p
}

// Baby steps: lane g owns j = g run + 1 .. g run + run.  Its first point is one short scalar multiplication, the rest
// of the run additions of G on the Jacobian point; the run is normalised with ONE inversion (as k_red shares one).
// Entries are inserted by 64-bit compare-and-swap with linear probing: the order of insertion varies from run to run,
// the SET of entries a probe sequence meets before its first empty slot does not.
template <class C, class F>
struct k_dlog_table {
  static __device__ __forceinline__ void run(size_t g, size_t total, const uint8_t* base, int run, unsigned log2_slots,
                                            unsigned long long* slots) {
  if (g >= total) return;
  Aff<F> G;
  aff_load<C>(G, base);
  Jac<F> cur;
  jac_smul_u64(cur, G, (uint64_t)g * run + 1);
  F xs[DLOG_RUN], zs[DLOG_RUN], pre[DLOG_RUN];
  F acc = one_of<F>();
  uint32_t inf = 0;  // j G = O: only a base of small order gets here; no entry
#pragma unroll 1
  for (int i = 0; i < run; i++) {
    if (i) jac_madd_edge(cur, cur, G);
    xs[i] = cur.x;
    zs[i] = cur.z;
    pre[i] = acc;
    if (gz_is_zero<C>(cur.z))
      inf |= 1u << i;
    else
      acc = mul(acc, cur.z);
  }
  F suf = inv(acc);
  const uint64_t mask = ((uint64_t)1 << log2_slots) - 1;
#pragma unroll 1
  for (int i = run - 1; i >= 0; i--) {
    if ((inf >> i) & 1) continue;
    F zi = mul(suf, pre[i]);  // 1 / z_i
    suf = mul(suf, zs[i]);
    const F x = mul(xs[i], sqr(zi));
    const uint64_t h = dlog_hash<C, F>(x);
    const unsigned long long v = ((h >> DLOG_JBITS) << DLOG_JBITS) | ((uint64_t)g * run + 1 + i);
    uint64_t idx = h & mask;
    for (uint64_t n = 0; n <= mask; n++) {  // (at most B of the 2 B slots are ever taken)
      if (atomicCAS(&slots[idx], 0ull, v) == 0ull) break;
      idx = (idx + 1) & mask;
    }
  }
}
};

// The launch-uniform giant steps: steps[i] = (i + 1) S G, i < K, normalised affine in the internal form
template <class C, class F>
__global__ void __launch_bounds__(64, GS_WPE) k_dlog_steps(const uint8_t* base, uint64_t S, int K, Aff<F>* steps) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= K) return;
  Aff<F> G, R;
  aff_load<C>(G, base);
  Jac<F> J;
  jac_smul_u64(J, G, (uint64_t)(i + 1) * S);
  jac_to_aff(R, J);
  steps[i] = R;
}

// The walk, one lane per point.  This launch covers the centres t0 .. t0 + nsteps - 1.  The lane keeps an affine anchor
// A = P - (c_t - S) G and takes K giant steps at a time: Q_(t+i-1) = A - M_i, M_i = i S G (launch-uniform, `steps`), all
// K slopes from ONE inversion of the product of the differences x(M_i) - x(A) (prefix products in LDS), x only; the last
// of them also gives y and becomes the next anchor.  Per step: 1 (prefix) + 2 (back-substitution) + 1 (slope) + 1
// (square) multiplications, + 1 for the canonical form that is hashed.
//   * x(M_i) = x(A): Q = O (x is the centre itself) or a doubling.  The difference is replaced by one so that the
//     shared product stays invertible, the step is flagged, the centre goes to the confirmation, no lookup.
//   * a hit gives the candidates c_t + j and c_t - j (only x is stored); each candidate inside [0, 2^bits) is confirmed
//     by x G == P.  Nothing is reported unconfirmed: a false hit, a wrong base, a point outside <G> cost time only.
//   * lanes that are done keep computing (the wave is in lockstep) but read and write nothing.
template <class C, class F>
struct k_dlog {
  static __device__ __forceinline__ void hit(bool& done, size_t g, const Aff<F>& G, const Aff<F>& P, int64_t x,
                                            unsigned bits, Fr<C>* out, uint8_t* found) {
    if (done || x < 0 || x >= ((int64_t)1 << bits)) return;
    if (!dlog_confirm<C, F>(G, P, (uint64_t)x)) return;
    Fr<C> k = fzero<FrM<C>>();
    k.v[0] = (uint32_t)x;
    k.v[1] = (uint32_t)((uint64_t)x >> 32);
    out[g] = to_mont(k);
    found[g] = 1;
    done = true;
  }
  static __device__ __forceinline__ void run(size_t g, size_t total, const uint8_t* pts, const uint8_t* base,
                                            const Aff<F>* steps, const unsigned long long* slots, unsigned log2_slots,
                                            unsigned log2_table, unsigned bits, unsigned fp_bits, uint64_t t0,
                                            uint32_t nsteps, int first, Fr<C>* out, uint8_t* found) {
  typedef DlogShape<F> SH;
  constexpr int K = SH::K, NW = SH::NW;
  __shared__ limb_t pre_s[K * NW * 64];
  limb_t* const mine = pre_s + (threadIdx.x & 63);
  const uint64_t B = (uint64_t)1 << log2_table, S = 2 * B;
  const uint64_t mask = ((uint64_t)1 << log2_slots) - 1, fpm = ((uint64_t)1 << fp_bits) - 1;
  bool done = g >= total;
  Aff<F> G, P;
  aff_load<C>(G, base);
  P = G;
  if (!done) {
    aff_load<C>(P, pts + g * AFFB(C, F));
    if (first) {
      const bool o = aff_is_inf(P);  // P = O: x = 0
      out[g] = fzero<FrM<C>>();
      found[g] = o ? 1 : 0;
      done = o;
    } else {
      done = found[g] != 0;
    }
  }
  // the anchor of the first block: P - (c_t0 - S) G = P + B G for t0 = 0
  Aff<F> A;
  {
    Jac<F> J;
    jac_smul_u64(J, G, t0 == 0 ? B : B + (t0 - 1) * S);
    if (t0 != 0) J.y = neg(J.y);
    jac_madd_edge(J, J, P);
    jac_to_aff(A, J);
    if (aff_is_inf(A)) done = true;  // x = c_(t0-1) (an earlier launch has reported it) or x = -B: not in range
  }
  uint32_t s = 0;
#pragma unroll 1
  while (s < nsteps) {
    if (__ballot(!done) == 0) break;
    const int kb = nsteps - s < (uint32_t)K ? (int)(nsteps - s) : K;  // launch-uniform
    F acc = one_of<F>();
    uint32_t zf = 0;
#pragma unroll 1
    for (int i = 1; i <= kb; i++) {
      F mx;
      ld_limbs(mx, &steps[i - 1].x);
      F d = norm(sub(mx, A.x));
      if (gz_is_zero<C>(d)) {
        zf |= 1u << i;
        d = one_of<F>();
      }
#pragma unroll
      for (int q = 0; q < NW; q++) mine[((i - 1) * NW + q) * 64] = reinterpret_cast<const limb_t*>(&acc)[q];
      acc = mul(acc, d);
    }
    F suf = inv(acc);
    Aff<F> An = A;
#pragma unroll 1
    for (int i = kb; i >= 1; i--) {
      F mx, my, pre;
      ld_limbs(mx, &steps[i - 1].x);
      ld_limbs(my, &steps[i - 1].y);
#pragma unroll
      for (int q = 0; q < NW; q++) reinterpret_cast<limb_t*>(&pre)[q] = mine[((i - 1) * NW + q) * 64];
      const bool z = ((zf >> i) & 1) != 0;
      F d = norm(sub(mx, A.x));
      if (z) d = one_of<F>();
      const F id = mul(suf, pre);  // 1 / (x(M_i) - x(A))
      suf = mul(suf, d);
      const F lam = mul(norm(sub(neg(my), A.y)), id);  // the chord through A and -M_i
      const F x3 = norm(sub(sub(sqr(lam), A.x), mx));
      if (i == K) {
        An.x = x3;
        An.y = norm(sub(mul(lam, norm(sub(A.x, x3))), A.y));
      }
      const uint64_t h = dlog_hash<C, F>(x3);
      const int64_t c = (int64_t)(B + (t0 + s + (uint64_t)(i - 1)) * S);
      if (done) continue;
      if (z) {
        hit(done, g, G, P, c, bits, out, found);
        continue;
      }
      const uint64_t fp = h >> DLOG_JBITS;
      uint64_t idx = h & mask;
      for (uint64_t n = 0; n <= mask && !done; n++) {  // to the first empty slot
        const unsigned long long v = slots[idx];
        if (v == 0) break;
        if ((((v >> DLOG_JBITS) ^ fp) & fpm) == 0) {
          const int64_t j = (int64_t)(v & (((uint64_t)1 << DLOG_JBITS) - 1));
          hit(done, g, G, P, c + j, bits, out, found);
          hit(done, g, G, P, c - j, bits, out, found);
        }
        idx = (idx + 1) & mask;
      }
    }
    if (kb == K) {
      if ((zf >> K) & 1) {  // A = +-M_K: the next anchor is O or 2 A, by the complete formulas
        Jac<F> J;
        jac_from_aff(J, A);
        Aff<F> m = steps[K - 1];
        m.y = neg(m.y);
        jac_madd_edge(J, J, m);
        jac_to_aff(An, J);
        if (aff_is_inf(An)) done = true;  // P = c G exactly and the centre c has just been tried
      }
      A = An;
    }
    s += (uint32_t)kb;
  }
}
};

// window tables: tab[(b*32 + w)*256 + d] = d * 2^(8w) * base[b]   (d = 0 -> identity)
template <class C, class F>
__global__ void __launch_bounds__(64, GS_WPE) k_build_tables(int nb, const uint8_t* bases, Aff<F>* tab) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)nb * 32 * 256) return;
  int d = (int)(i & 255), w = (int)((i >> 8) & 31), b = (int)(i >> 13);
  Fr<C> k = fzero<FrM<C>>();
  k.v[w >> 2] = (uint32_t)d << ((w & 3) * 8);
  Aff<F> B;
  aff_load<C>(B, bases + b * AFFB(C, F));
  Jac<F> J;
  jac_smul(J, B, k);  // integer multiple d*2^(8w) may exceed r: plain path (endo decomposition assumes k < r)
  Aff<F> R;
  jac_to_aff(R, J);
  tab[i] = R;
}

// Second level: 16-bit windows, tab16[(b*16 + w)*65536 + d] = d * 2^(16w) * base[b], each entry the sum of two
// first-level entries (one mixed addition per entry, one inversion per 16 entries).  1.8 GB per CRS for both groups -- a
// fixed-base scalar then costs 16 mixed additions instead of 32.  288 GB of HBM is what makes this the right trade.
template <class C, class F>
__global__ void __launch_bounds__(64, GS_WPE) k_build_tables16(int nb, const Aff<F>* tab8, Aff<F>* tab16) {
  // one lane = 16 consecutive entries (same base, window and high byte), normalised with ONE inversion
  constexpr int G = 16;
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)nb * 16 * 65536 / G) return;
  size_t i0 = g * G;
  uint32_t d0 = (uint32_t)(i0 & 65535u);
  int w = (int)((i0 >> 16) & 15), b = (int)(i0 >> 20);
  Aff<F> hi = tab8[((size_t)b * 32 + 2 * w + 1) * 256 + (d0 >> 8)];
  Jac<F> J[G];
  F pre[G];
  F acc = one_of<F>();
  for (int t = 0; t < G; t++) {
    Aff<F> lo = tab8[((size_t)b * 32 + 2 * w) * 256 + ((d0 + t) & 255u)];
    jac_from_aff(J[t], lo);
    jac_madd(J[t], J[t], hi);
    pre[t] = acc;
    if (!is_zero_limbs(J[t].z)) acc = mul(acc, J[t].z);
  }
  F inv_all = inv(acc);
  for (int t = G - 1; t >= 0; t--) {
    Aff<F> R;
    if (is_zero_limbs(J[t].z)) {
      R.x = zero_of<F>();
      R.y = zero_of<F>();
    } else {
      F zi = mul(inv_all, pre[t]);
      inv_all = mul(inv_all, J[t].z);
      jac_to_aff_zinv(R, J[t], zi);
    }
    tab16[i0 + t] = R;
  }
}

// --------------------------------------------------------------------------
// Fr preparation for prove (one lane per equation)
// --------------------------------------------------------------------------
template <class C>
struct k_prep_prove {
  static __device__ __forceinline__ void run(size_t e_in, size_t N, int m, int n, int kx, int ky, const Fr<C>* G, const Fr<C>* R, const Fr<C>* S,
                 const Fr<C>* T, const Fr<C>* xs, const Fr<C>* ys, const Fr<C>* as, const Fr<C>* bs, PoolMap pm,
                 Fr<C>* pool, int shared_vars) {
  size_t e = e_in;
  if (e >= N) return;
  typedef Fr<C> S_;
  // shared_vars: a Statement -- every equation of the batch is over the SAME variables (and commit randomness)
  const size_t ev = shared_vars ? 0 : e;
  G += e * m * n;
  R += ev * m * kx;
  S += ev * n * ky;
  T += e * ky * kx;
  if (xs) xs += ev * m;
  if (ys) ys += ev * n;
  if (as) as += e * n;
  if (bs) bs += e * m;
  S_* P = pool + e * pm.total;
  for (int i = 0; i < m * kx; i++) P[pm.RC + i] = from_mont(R[i]);
  for (int i = 0; i < n * ky; i++) P[pm.SC + i] = from_mont(S[i]);
  for (int i = 0; i < ky * kx; i++) P[pm.TC + i] = from_mont(T[i]);
  if (xs)
    for (int i = 0; i < m; i++) P[pm.XC + i] = from_mont(xs[i]);
  if (ys)
    for (int j = 0; j < n; j++) P[pm.YC + j] = from_mont(ys[j]);
  // Psi = R^T Gamma (kx x n); Omega = Psi S - T^T (kx x ky); rho_k (scalar-Y types)
  for (int k = 0; k < kx; k++) {
    S_ om[2] = {fzero<FrM<C>>(), fzero<FrM<C>>()};
    S_ rho = fzero<FrM<C>>();
    for (int j = 0; j < n; j++) {
      S_ psi = fzero<FrM<C>>();
      for (int i = 0; i < m; i++) psi = add(psi, mul(R[i * kx + k], G[i * n + j]));
      P[pm.PSI + k * n + j] = from_mont(psi);
      for (int l = 0; l < ky; l++) om[l] = add(om[l], mul(psi, S[j * ky + l]));
      if (ys) rho = add(rho, mul(psi, ys[j]));
    }
    for (int l = 0; l < ky; l++) P[pm.OM + k * ky + l] = from_mont(sub(om[l], T[l * kx + k]));
    if (bs) {
      for (int i = 0; i < m; i++) rho = add(rho, mul(R[i * kx + k], bs[i]));
      P[pm.RHO + k] = from_mont(rho);
    }
  }
  // Phi = S^T Gamma^T (ky x m); sigma_l (scalar-X types)
  for (int l = 0; l < ky; l++) {
    S_ sig = fzero<FrM<C>>();
    for (int i = 0; i < m; i++) {
      S_ phi = fzero<FrM<C>>();
      for (int j = 0; j < n; j++) phi = add(phi, mul(S[j * ky + l], G[i * n + j]));
      P[pm.PHI + l * m + i] = from_mont(phi);
      if (xs) sig = add(sig, mul(phi, xs[i]));
    }
    if (as) {
      for (int j = 0; j < n; j++) sig = add(sig, mul(S[j * ky + l], as[j]));
      P[pm.SIG + l] = from_mont(sig);
    }
  }
}
};

// The same for large arities (m n in the thousands and beyond, benches/bench.rs:451-498 uses 334 x 334): one lane per
// OUTPUT SCALAR instead of one per equation.  Phase a: conversions and the two matrix products (a lane = one entry
// of Psi or Phi = one inner product); phase b: the <= 8 scalars per equation that depend on Psi / Phi.
template <class C>
struct k_prep_prove_wide_a {
  static __device__ __forceinline__ void run(size_t g, size_t total, int W, int m, int n, int kx, int ky, const Fr<C>* G, const Fr<C>* R,
                        const Fr<C>* S, const Fr<C>* T, const Fr<C>* xs, const Fr<C>* ys, PoolMap pm, Fr<C>* pool,
                        int shared_vars) {
  if (g >= total) return;
  size_t e = g / W;
  int w = (int)(g % W);
  typedef Fr<C> S_;
  const size_t ev = shared_vars ? 0 : e;
  G += e * m * n;
  R += ev * m * kx;
  S += ev * n * ky;
  T += e * ky * kx;
  if (xs) xs += ev * m;
  if (ys) ys += ev * n;
  S_* P = pool + e * pm.total;
  int o = 0;
  if (w < o + m * kx) { P[pm.RC + w - o] = from_mont(R[w - o]); return; }
  o += m * kx;
  if (w < o + n * ky) { P[pm.SC + w - o] = from_mont(S[w - o]); return; }
  o += n * ky;
  if (w < o + ky * kx) { P[pm.TC + w - o] = from_mont(T[w - o]); return; }
  o += ky * kx;
  if (w < o + m) { if (xs) P[pm.XC + w - o] = from_mont(xs[w - o]); return; }
  o += m;
  if (w < o + n) { if (ys) P[pm.YC + w - o] = from_mont(ys[w - o]); return; }
  o += n;
  if (w < o + kx * n) {  // Psi[k][j] = sum_i R[i][k] G[i][j]
    int k = (w - o) / n, j = (w - o) % n;
    S_ psi = fzero<FrM<C>>();
    for (int i = 0; i < m; i++) psi = add(psi, mul(R[i * kx + k], G[i * n + j]));
    P[pm.PSI + k * n + j] = from_mont(psi);
    return;
  }
  o += kx * n;
  if (w < o + ky * m) {  // Phi[l][i] = sum_j S[j][l] G[i][j]
    int l = (w - o) / m, i = (w - o) % m;
    S_ phi = fzero<FrM<C>>();
    for (int j = 0; j < n; j++) phi = add(phi, mul(S[j * ky + l], G[i * n + j]));
    P[pm.PHI + l * m + i] = from_mont(phi);
  }
}
};
template <class C>
struct k_prep_prove_wide_b {
  static __device__ __forceinline__ void run(size_t g, size_t total, int m, int n, int kx, int ky, const Fr<C>* R, const Fr<C>* S, const Fr<C>* T,
                        const Fr<C>* xs, const Fr<C>* ys, const Fr<C>* as, const Fr<C>* bs, PoolMap pm, Fr<C>* pool,
                        int shared_vars) {
  if (g >= total) return;
  const int W = kx * ky + kx + ky;
  size_t e = g / W;
  int w = (int)(g % W);
  typedef Fr<C> S_;
  const size_t ev = shared_vars ? 0 : e;
  R += ev * m * kx;
  S += ev * n * ky;
  T += e * ky * kx;
  if (xs) xs += ev * m;
  if (ys) ys += ev * n;
  if (as) as += e * n;
  if (bs) bs += e * m;
  S_* P = pool + e * pm.total;
  if (w < kx * ky) {  // Omega[k][l] = sum_j Psi[k][j] S[j][l] - T[l][k]
    int k = w / ky, l = w % ky;
    S_ om = fzero<FrM<C>>();
    for (int j = 0; j < n; j++) om = add(om, mul(to_mont(P[pm.PSI + k * n + j]), S[j * ky + l]));
    P[pm.OM + k * ky + l] = from_mont(sub(om, T[l * kx + k]));
  } else if (w < kx * ky + kx) {  // rho_k = sum_j Psi[k][j] y_j + sum_i R[i][k] b_i   (scalar-Y types)
    int k = w - kx * ky;
    if (!bs) return;
    S_ rho = fzero<FrM<C>>();
    if (ys)
      for (int j = 0; j < n; j++) rho = add(rho, mul(to_mont(P[pm.PSI + k * n + j]), ys[j]));
    for (int i = 0; i < m; i++) rho = add(rho, mul(R[i * kx + k], bs[i]));
    P[pm.RHO + k] = from_mont(rho);
  } else {  // sigma_l = sum_i Phi[l][i] x_i + sum_j S[j][l] a_j   (scalar-X types)
    int l = w - kx * ky - kx;
    if (!as) return;
    S_ sig = fzero<FrM<C>>();
    if (xs)
      for (int i = 0; i < m; i++) sig = add(sig, mul(to_mont(P[pm.PHI + l * m + i]), xs[i]));
    for (int j = 0; j < n; j++) sig = add(sig, mul(S[j * ky + l], as[j]));
    P[pm.SIG + l] = from_mont(sig);
  }
}
};
// out[e * out_stride + i] = canonical(in[e * cnt + i]): the Gamma conversion of the verifier, one lane per scalar
template <class C>
struct k_fr_canonical {
  static __device__ __forceinline__ void run(size_t g, size_t total, int cnt, const Fr<C>* in, int out_stride, Fr<C>* out) {
  if (g >= total) return;
  size_t e = g / cnt;
  int i = (int)(g % cnt);
  out[e * out_stride + i] = from_mont(in[g]);
}
};

// canonical -> Montgomery boundary form (gs_fr_matmul hands the prover's canonical products back as Fr values)
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_fr_to_mont(size_t total, const Fr<C>* in, Fr<C>* out) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  out[g] = to_mont(in[g]);
}

// Fr preparation for verify: Gamma (and scalar constants / target) -> canonical
template <class C>
struct k_prep_verify {
  static __device__ __forceinline__ void run(size_t e_in, size_t N, int m, int n, const Fr<C>* G, const Fr<C>* as,
                                                    const Fr<C>* bs, const Fr<C>* tq, PoolMap pm, Fr<C>* pool) {
  size_t e = e_in;
  if (e >= N) return;
  Fr<C>* P = pool + e * pm.total;
  if (G)  // (large arities convert Gamma with k_fr_canonical, one lane per scalar)
    for (int i = 0; i < m * n; i++) P[pm.GC + i] = from_mont(G[e * m * n + i]);
  if (as)
    for (int j = 0; j < n; j++) P[pm.AC + j] = from_mont(as[e * n + j]);
  if (bs)
    for (int i = 0; i < m; i++) P[pm.BC + i] = from_mont(bs[e * m + i]);
  if (tq) P[pm.NT] = from_mont(neg(tq[e]));
}
};

template <class C> GS_HD_NOINLINE void f12_pow_u64(Fp12<C>& r, const Fp12<C>& b, uint64_t k) {
  Fp12<C> acc;
  f12_one(acc);
  bool started = false;
  for (int i = 63; i >= 0; i--) {
    if (started) f12_sqr(acc, acc);
    if ((k >> i) & 1) {
      if (started)
        f12_mul(acc, acc, b);
      else
        acc = b;
      started = true;
    }
  }
  r = acc;
}

// Fr preparation for the batched verifier with the random exponents folded into the G1
// arguments: rho[e][2a+b] (64-bit) -> canonical RH[2a+b]; x-scalar types also need
// a_j*rho_ab (AR[(j*2+a)*2+b]); QuadEqu needs (-t)*rho_ab (NR[a*2+b]).
template <class C>
__global__ void __launch_bounds__(64, GS_WPE)
    k_prep_verify_rlc(size_t N, int m, int n, const Fr<C>* G, const Fr<C>* as, const Fr<C>* bs, const Fr<C>* tq,
                      const uint64_t* rho, PoolMap pm, Fr<C>* pool) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  Fr<C>* P = pool + e * pm.total;
  if (G)
    for (int i = 0; i < m * n; i++) P[pm.GC + i] = from_mont(G[e * m * n + i]);
  if (bs)
    for (int i = 0; i < m; i++) P[pm.BC + i] = from_mont(bs[e * m + i]);
  Fr<C> rm[4];
  for (int c = 0; c < 4; c++) {
    Fr<C> r = fzero<FrM<C>>();
    uint64_t v = rho[e * 4 + c];
    r.v[0] = (uint32_t)v;
    r.v[1] = (uint32_t)(v >> 32);
    P[pm.RH + c] = r;      // canonical (rho < 2^64 < r)
    rm[c] = to_mont(r);
  }
  if (as)
    for (int j = 0; j < n; j++)
      for (int c = 0; c < 4; c++) P[pm.AR + j * 4 + c] = from_mont(mul(as[e * n + j], rm[c]));
  if (tq) {
    Fr<C> nt = neg(tq[e]);
    for (int c = 0; c < 4; c++) P[pm.NR + c] = from_mont(mul(nt, rm[c]));
  }
}

// out_t[e] = t_e^(rho[e][3]) for the PPE target cell (boundary in, internal out)
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_rlc_tpow(size_t N, const uint8_t* target, const uint64_t* rho,
                                                 Fp12<C>* out_t) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  Fp12<C> t, h;
  f12_from_boundary<C>(t, reinterpret_cast<const BFq<C>*>(target) + 12 * e);
  f12_pow_u64(h, t, rho[e * 4 + 3]);
  out_t[e] = h;
}

// ---- one equation, N proofs (gs_verify_equation_rlc) -------------------------------------------------
// Fr preparation.  The constants exist ONCE, so the scalars live in two pools:
//   per proof (pm.total scalars each):  RH[2a + b] = rho[e][2a + b];  AR[4j + 2a + b] = a_j rho_e,ab (scalar a only)
//   shared (one copy, k_prep_verify_eq_rlc_shared): Gamma, b, the sums r_ab and -t r_ab
// The sums r_ab = sum_e rho_e,ab are taken here as well, because a _dev caller's rho is device memory: every wave adds
// the low and the high 32-bit halves of its 64 exponents separately into sums[2c], sums[2c + 1] (u64 each: exact below
// 2^32 proofs, whatever order the atomics land in), and the shared kernel puts the halves together.
template <class C>
__global__ void __launch_bounds__(64, GS_WPE)
    k_prep_verify_eq_rlc(size_t N, int n, const Fr<C>* as, const uint64_t* rho, PoolMap pm, Fr<C>* pool,
                         unsigned long long* sums) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = e < N;
  unsigned long long part[8];
  Fr<C> rm[4];
  for (int c = 0; c < 4; c++) {
    uint64_t v = live ? rho[e * 4 + c] : 0;
    part[2 * c] = v & 0xFFFFFFFFull;
    part[2 * c + 1] = v >> 32;
    Fr<C> r = fzero<FrM<C>>();
    r.v[0] = (uint32_t)v;
    r.v[1] = (uint32_t)(v >> 32);
    if (live) pool[e * pm.total + pm.RH + c] = r;  // canonical (rho < 2^64 < r)
    rm[c] = to_mont(r);
  }
  if (live && as)
    for (int j = 0; j < n; j++)
      for (int c = 0; c < 4; c++) pool[e * pm.total + pm.AR + j * 4 + c] = from_mont(mul(as[j], rm[c]));
  for (int k = 0; k < 8; k++) {  // (every lane of the wave takes part: lanes past N hold zeros)
    unsigned long long v = part[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (threadIdx.x == 0 && v) atomicAdd(sums + k, v);
  }
}
// the shared pool: lane g converts Gamma[g] and b[g]; lane 0 also assembles r_c = sums[2c] + 2^32 sums[2c + 1] (below
// 2^96) as a canonical Fr (RH) and, for QuadEqu, NR[c] = -t r_c
template <class C>
__global__ void __launch_bounds__(64, GS_WPE)
    k_prep_verify_eq_rlc_shared(int m, int n, const Fr<C>* G, const Fr<C>* bs, const Fr<C>* tq,
                                const unsigned long long* sums, PoolMap pm, Fr<C>* pool) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < (size_t)m * n) pool[pm.GC + g] = from_mont(G[g]);
  if (bs && g < (size_t)m) pool[pm.BC + g] = from_mont(bs[g]);
  if (g != 0) return;
  for (int c = 0; c < 4; c++) {
    const unsigned long long lo = sums[2 * c], hi = sums[2 * c + 1];
    const unsigned long long w0 = lo + (hi << 32), w1 = (hi >> 32) + (w0 < lo ? 1ull : 0ull);
    Fr<C> r = fzero<FrM<C>>();
    r.v[0] = (uint32_t)w0;
    r.v[1] = (uint32_t)(w0 >> 32);
    r.v[2] = (uint32_t)w1;
    r.v[3] = (uint32_t)(w1 >> 32);
    pool[pm.RH + c] = r;
    if (tq) pool[pm.NR + c] = from_mont(mul(neg(tq[0]), to_mont(r)));
  }
}
// t^(r_11): ONE power for the whole batch (PPE; boundary in, internal out).  The exponent is the canonical r_11 of the
// shared pool (below 2^96); general squarings, as k_rlc_tpow: the target is raised without a subgroup check.
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_eq_rlc_tpow(const uint8_t* target, const Fr<C>* r11, Fp12<C>* out_t) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Fp12<C> t, acc;
  f12_from_boundary<C>(t, reinterpret_cast<const BFq<C>*>(target));
  const Fr<C> k = r11[0];
  f12_one(acc);
  bool started = false;
  for (int i = 127; i >= 0; i--) {
    if (started) f12_sqr(acc, acc);
    if ((k.v[i >> 5] >> (i & 31)) & 1) {
      if (started)
        f12_mul(acc, acc, t);
      else
        acc = t;
      started = true;
    }
  }
  out_t[0] = acc;
}
// Segmented K-ary sum ACROSS the batch.  The input is `n_in` rows of `cols` points (column q of every row is summed
// with column q of the others); lane (r, q) sums rows [K r, K r + K) of column q into a Jacobian partial, and the host
// repeats the launch on its own output until one row is left, which k_red normalises with one shared inversion.  Level
// 0 reads affine boundary points (`aff`, `row_bytes` apart; mixed additions), the levels above read the partials.
// jac_madd / jac_add are the complete forms: identities, equal operands (a doubling) and opposite ones (the identity,
// Z = 0 exactly) come out right at every level.
template <class C, class F>
struct k_batch_sum {
  static __device__ __forceinline__ void run(size_t g, size_t total, size_t n_in, int cols, const uint8_t* aff,
                                             uint32_t row_bytes, const Jac<F>* jin, Jac<F>* out, int K) {
  if (g >= total) return;
  const size_t r = g / cols, q = g % cols;
  const size_t lo = r * (size_t)K, hi = lo + K < n_in ? lo + K : n_in;
  Jac<F> s;
  if (aff) {
    Aff<F> a;
    aff_load<C>(a, aff + lo * (size_t)row_bytes + q * AFFB(C, F));
    jac_from_aff(s, a);
    for (size_t i = lo + 1; i < hi; i++) {
      aff_load<C>(a, aff + i * (size_t)row_bytes + q * AFFB(C, F));
      jac_madd(s, s, a);
    }
  } else {
    s = jin[lo * cols + q];
    for (size_t i = lo + 1; i < hi; i++) jac_add(s, s, jin[i * cols + q]);
  }
  out[r * cols + q] = s;
}
};

// --------------------------------------------------------------------------
// linear-combination engine
// --------------------------------------------------------------------------
template <class C, class F, bool ENDO = true>
struct k_var {
  static __device__ __forceinline__ void run(size_t g, size_t total, int ntask, const VarTask* tasks, ArrTab arrs,
                                            const Fr<C>* pool, int pool_n, Jac<F>* part, int nslots) {
  if (g >= total) return;
  size_t e = g / ntask;
  VarTask t = tasks[g % ntask];
  Fr<C> k = pool[e * pool_n + t.s_idx];
  Aff<F> P;
  aff_load<C>(P, arrs.base[t.p_arr] + e * arrs.stride[t.p_arr] + (size_t)t.p_idx * AFFB(C, F));
  if (t.neg) P.y = neg(P.y);
  Jac<F> J;
  jac_smul_any<C, F, ENDO>(J, P, k);
  part[e * nslots + t.slot] = J;
}
};

// joint MSM: one lane = one GrpTask (<= TMAX bases sharing a doubling chain; the lane's table build serves all of the
// group's outputs, which run one after the other)
// WPE2 = 2 (G1 only): the kernel is built for TWO waves per SIMD.  With the point operations as register-only
// subroutines (gs_pointops_asm.h: v48 .. v206 on BLS12-381) the whole lane fits 256 registers, and a second resident
// wave issues into every slot the first one leaves empty -- at one wave per SIMD a v_mad_u64_u32 issues every ~5.9
// cycles and a full-rate instruction every ~5.3, at two every ~4.75 / ~2.7 (tools/ubench.hip, profiles/r4/).  Planned
// when the launch has enough waves to put two on every SIMD (csrc/gs_amd.hip, var_w2).
template <class C, class F, int TMAX, int W, int WPE2 = 1>
struct k_var_multi {
  static constexpr int WPE = WPE2;
  static __device__ __forceinline__ void run(size_t w_in, size_t total, int ngrp, const GrpTask* grps, const VarTask* tasks,
                                                  ArrTab arrs, const Fr<C>* pool, int pool_n, Jac<F>* part,
                                                  int nslots, size_t g0, Aff<F>* tabws) {
  size_t w = w_in;  // lane within this launch = its slot in `tabws`
  size_t g = g0 + w;
  if (g >= total) return;
  size_t e = g / ngrp;
  GrpTask gt = grps[g % ngrp];
  // the lane's workspace: its affine table, then the Jacobian staging of the build (STRAUS_WS_BYTES per lane)
  constexpr size_t NTAB = (size_t)TMAX << (W - 1);
  uint8_t* ws = reinterpret_cast<uint8_t*>(tabws) + w * (NTAB * (sizeof(Aff<F>) + sizeof(Jac<F>)));
  Aff<F>* at = reinterpret_cast<Aff<F>*>(ws);
  Jac<F>* jt = reinterpret_cast<Jac<F>*>(ws + NTAB * sizeof(Aff<F>));
  F zback;
  {
    Aff<F> P[TMAX];
    for (uint32_t i = 0; i < gt.nt; i++) {
      VarTask t = tasks[gt.first[0] + i];
      aff_load<C>(P[i], arrs.base[t.p_arr] + e * arrs.stride[t.p_arr] + (size_t)t.p_idx * AFFB(C, F));
      if (t.neg) P[i].y = neg(P[i].y);
    }
    unsigned long long sb0 = GS_STAMP_T();
    jac_straus_build<C, F, TMAX, W>(at, zback, P, (int)gt.nt, jt);
    GS_STAMP_ADD(5, GS_STAMP_T() - sb0);
  }
  for (uint32_t o = 0; o < gt.no; o++) {
    Fr<C> k[TMAX];
    for (uint32_t i = 0; i < gt.nt; i++) k[i] = pool[e * pool_n + tasks[gt.first[o] + i].s_idx];
    Jac<F> J;
    jac_straus_run<C, F, TMAX, W, true, (WPE2 == 2 ? 18 : 36)>(J, k, (int)gt.nt, at, zback);
    part[e * nslots + gt.slot[o]] = J;
  }
}
};

// ---- large arities: window tables of the BASES, shared by every output that uses them --------------------------------
// The verifier's Gamma^T c is 2 n outputs over the SAME 2 m commitment components (benches/bench.rs:451-498: m = n = 334).
// A Straus lane builds its own tables (8 bases x 16 entries, shared by at most 4 outputs); with hundreds of outputs per
// base it pays to build ONE wide table per (equation, base) -- 2^(W-1) = 128 true-affine multiples for 8-bit signed
// windows, one inversion per base -- and let every output's lanes read them: 2 x 17 look-ups and mixed additions per
// term instead of 2 x 27, one shared doubling chain of 128 instead of 130 doublings, no per-lane build at all.
template <class C, class F, int W>
struct k_tab_build {
  static __device__ __forceinline__ void run(size_t g, size_t total, int nb, ArrTab arrs, int arr, Jac<F>* stage, Aff<F>* tabs) {
  if (g >= total) return;
  constexpr int NE = 1 << (W - 1);
  size_t e = g / nb;
  int b = (int)(g % nb);
  Aff<F> P;
  aff_load<C>(P, arrs.base[arr] + e * arrs.stride[arr] + (size_t)b * AFFB(C, F));
  smul_affine_table(tabs + g * NE, stage + g * NE, P, NE);
}
};
// one lane = one GrpTask as in k_var_multi (<= TMAX terms sharing the doubling chain, `no` outputs one after the other);
// base t of the group is entry tasks[..].p_idx of array 0, its table tabs[(e * nb + p_idx) * NE ..]
template <class C, class F, int TMAX, int W>
struct k_var_tab {
  static __device__ __forceinline__ void run(size_t g, size_t total, int ngrp, const GrpTask* grps, const VarTask* tasks,
                                              const Fr<C>* pool, int pool_n, Jac<F>* part, int nslots, const Aff<F>* tabs,
                                              int nb) {
  if (g >= total) return;
  constexpr int NE = 1 << (W - 1);
  size_t e = g / ngrp;
  GrpTask gt = grps[g % ngrp];
  for (uint32_t o = 0; o < gt.no; o++) {
    Fr<C> k[TMAX];
    const Aff<F>* tp[TMAX];
    uint32_t negm = 0;
    for (uint32_t i = 0; i < gt.nt; i++) {
      VarTask t = tasks[gt.first[o] + i];
      k[i] = pool[e * pool_n + t.s_idx];
      tp[i] = tabs + (e * (size_t)nb + t.p_idx) * NE;
      if (t.neg) negm |= 1u << i;
    }
    Jac<F> J;
    jac_straus_run<C, F, TMAX, W, true>(J, k, (int)gt.nt, (const Aff<F>*)nullptr, one_of<F>(), tp, negm);
    part[e * nslots + gt.slot[o]] = J;
  }
}
};

template <class C, class F>
struct k_fix {
  static __device__ __forceinline__ void run(size_t g, size_t total, int ntask, const FixTask* tasks, ArrTab arrs,
                                            const Fr<C>* pool, int pool_n, const Aff<F>* tab, Jac<F>* part,
                                            int nslots) {
  if (g >= total) return;
  size_t e = g / ntask;
  FixTask t = tasks[g % ntask];
  Jac<F> acc;
  jac_set_inf(acc);
  // 2 x 16 window look-ups (16-bit windows, k_build_tables16) and the optional affine addend = up to 33 mixed
  // additions.  The tables are 0.6 / 1.2 GB per CRS: every look-up is an HBM access, and at one wave per SIMD its whole
  // latency is exposed unless it was requested a step ahead -- so the entry of step j + 1 is loaded (global_load:
  // vmcnt only) before the addition of step j starts; the running sum is updated in place (G1: the register-only
  // subroutines of gs_pointops_asm.h) and never has its address taken.
  typedef const __attribute__((address_space(1))) limb_t* gptr;
  auto ldaff = [](const Aff<F>* p) -> Aff<F> {
    Aff<F> v;
    constexpr int NWD = (int)(sizeof(Aff<F>) / sizeof(limb_t));
    gptr w = (gptr) reinterpret_cast<const limb_t*>(p);
#pragma unroll
    for (int q = 0; q < NWD; q++) reinterpret_cast<limb_t*>(&v)[q] = w[q];
    return v;
  };
  Fr<C> k0, k1;  // the (<= 2) scalars of this lane; an absent term keeps zero digits
  for (int i = 0; i < FrM<C>::N; i++) k0.v[i] = k1.v[i] = 0;
  if (t.t0 != 0xFF) k0 = pool[e * pool_n + t.s0];
  if (t.t1 != 0xFF) k1 = pool[e * pool_n + t.s1];
  auto slot = [&](int j) -> const Aff<F>* {  // j = term * 16 + window; nullptr = nothing to add
    const int term = j >> 4, w = j & 15;
    const Fr<C>& k = term ? k1 : k0;
    const uint32_t d = (k.v[w >> 1] >> ((w & 1) * 16)) & 65535u;
    const int tb = term ? t.t1 : t.t0;
    if (d == 0 || tb == 0xFF) return nullptr;
    return tab + ((size_t)tb * 16 + (size_t)w) * 65536 + d;
  };
  const Aff<F>* cur = slot(0);
  Aff<F> q = ldaff(cur ? cur : tab);
#pragma unroll 1
  for (int j = 0; j < 32; j++) {
    const Aff<F>* nxt = j + 1 < 32 ? slot(j + 1) : nullptr;
    Aff<F> qn = ldaff(nxt ? nxt : tab);  // (a step without a look-up requests entry 0: harmless, never used)
    if (cur) jac_madd_ip(acc, q);
    q = qn;
    cur = nxt;
  }
  if (t.a_arr != 0xFF) {
    Aff<F> a;
    aff_load<C>(a, arrs.base[t.a_arr] + e * arrs.stride[t.a_arr] + (size_t)t.a_idx * AFFB(C, F));
    if (t.a_neg) a.y = neg(a.y);
    jac_madd_ip(acc, a);
  }
  part[e * nslots + t.slot] = acc;
}
};

// One lane = up to RED_K consecutive outputs (two points each) and ONE inversion for all of them (Montgomery's trick
// over their Z coordinates): the inversion is most of this kernel (496 of ~530 Fq multiplications per output in G1).
constexpr int RED_K = 8;
template <class C, class F>
struct k_red {
  static __device__ __forceinline__ void run(size_t g, size_t total, int ntask, const RedTask* tasks, const Jac<F>* part,
                                            int nslots, OutTab outs, int K) {
  if (g >= total) return;
  const int nl = (ntask + K - 1) / K;  // lanes per equation
  size_t e = g / nl;
  int t0 = (int)(g % nl) * K, nt = ntask - t0 < K ? ntask - t0 : K;
  const Jac<F>* P = part + e * nslots;
  Jac<F> s[2 * RED_K];
  F pre[2 * RED_K];  // pre[i] = z_0 ... z_(i-1) (identities count as 1)
  F acc = one_of<F>();
  for (int k = 0; k < nt; k++) {
    RedTask t = tasks[t0 + k];
    Jac<F> s0 = P[t.b0], s1 = P[t.b1];
    for (uint32_t i = t.b0 + 1; i < t.e0; i++) jac_add(s0, s0, P[i]);
    for (uint32_t i = t.b1 + 1; i < t.e1; i++) jac_add(s1, s1, P[i]);
    s[2 * k] = s0;
    s[2 * k + 1] = s1;
    pre[2 * k] = acc;
    if (!is_zero_limbs(s0.z)) acc = mul(acc, s0.z);
    pre[2 * k + 1] = acc;
    if (!is_zero_limbs(s1.z)) acc = mul(acc, s1.z);
  }
  F suf = inv(acc);  // 1 / (z_0 ... z_(2 nt - 1))
  for (int i = 2 * nt - 1; i >= 0; i--) {
    RedTask t = tasks[t0 + i / 2];
    Aff<F> a;
    F zi = mul(suf, pre[i]);  // 1 / z_i
    if (!is_zero_limbs(s[i].z)) suf = mul(suf, s[i].z);
    jac_to_aff_zinv(a, s[i], zi);  // (identity -> (0, 0), zi unused)
    uint8_t* o = outs.base[t.out_arr] + e * outs.stride[t.out_arr] + (2 * (size_t)t.out_idx + (i & 1)) * AFFB(C, F);
    aff_store<C>(o, a);
  }
}
};

// Large arities (benches/bench.rs:451-498, m = n = 334): an output is the sum of hundreds of partial slots.  k_red
// folds its slots serially in ONE lane, so the host first folds runs of K slots in parallel (one lane per run), and
// again, until every run k_red sees is short: a segmented K-ary tree reduction.
struct FoldTask {
  uint32_t lo, hi, dst, pad;  // dst slot (in the output array) <- sum of input slots [lo, hi)
};
template <class C, class F>
struct k_slot_fold {
  static __device__ __forceinline__ void run(size_t g, size_t total, int ntask, const FoldTask* tasks, const Jac<F>* in,
                                                          int ns_in, Jac<F>* out, int ns_out) {
  if (g >= total) return;
  size_t e = g / ntask;
  FoldTask t = tasks[g % ntask];
  const Jac<F>* P = in + e * ns_in;
  Jac<F> s = P[t.lo];
  for (uint32_t i = t.lo + 1; i < t.hi; i++) jac_add(s, s, P[i]);
  out[e * ns_out + t.dst] = s;
}
};

// --------------------------------------------------------------------------
// pairing side
// --------------------------------------------------------------------------
// Line tables of the six CRS G2 points (v0.0 v0.1 v1.0 v1.1 W2.0 W2.1), built once per CRS: one lane per point.
template <class C> __global__ void __launch_bounds__(64, GS_WPE) k_line_tables(const uint8_t* crs_g2, Line<C>* out) {
  int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= 6) return;
  Aff<Fp2<C>> q;
  aff_load<C>(q, crs_g2 + (size_t)i * AFFB(C, Fp2<C>));
  miller_line_table<C>(out + (size_t)i * miller_line_count<C>(), q);
}

// Lanes are TASK-MAJOR: lane g works on task g / N of equation g % N, so a wave holds 64 equations of one task and its
// lanes agree on the number of pairs and on which of them read line tables (`ltab`, pairs with Q array 2 = CRS).
template <class C, bool TWIN>
struct k_miller {
  static __device__ __forceinline__ void run(size_t g, size_t total, int ntask, const MillerTask* tasks, ArrTab parr,
                                               ArrTab qarr, Fp12<C>* out, int ostride, const Line<C>* ltab) {
  if (g >= total) return;
  const size_t N = total / ntask;
  const size_t ti = g / N, e = g % N;
  const size_t go = e * ntask + ti;  // partials stay equation-major for k_final
  MillerTask t = tasks[ti];
  Aff<Fq<C>> p0[MILLER_CH];
  Aff<Fp2<C>> qs[MILLER_CH];
  Proj2<C> ts[MILLER_CH];
  const Line<C>* fx[MILLER_CH];
  bool anyfx = false;  // uniform over the wave (task-major lanes)
  for (int k = 0; k < t.np; k++) {
    fx[k] = (ltab && t.pr[k].q_arr == 2) ? ltab + (size_t)t.pr[k].q_idx * miller_line_count<C>() : nullptr;
    anyfx |= fx[k] != nullptr;
  }
  if constexpr (TWIN) {
    Aff<Fq<C>> p1[MILLER_CH];
    uint8_t live[MILLER_CH];
    for (int k = 0; k < t.np; k++) {
      PairRef r = t.pr[k];
      const uint8_t* pb = parr.base[r.p_arr] + e * parr.stride[r.p_arr] + (size_t)r.p_idx * AFFB(C, Fq<C>);
      aff_load<C>(p0[k], pb);
      aff_load<C>(p1[k], pb + AFFB(C, Fq<C>));
      aff_load<C>(qs[k], qarr.base[r.q_arr] + e * qarr.stride[r.q_arr] + (size_t)r.q_idx * AFFB(C, Fp2<C>));
      if (r.neg) {
        p0[k].y = neg(p0[k].y);
        p1[k].y = neg(p1[k].y);
      }
    }
    Fp12<C> f0, f1;
    multi_miller2(f0, f1, p0, p1, qs, t.np, ts, live, anyfx ? fx : nullptr);
    out[2 * go] = f0;      // cell (0, b)
    out[2 * go + 1] = f1;  // cell (1, b)
  } else {
    bool live[MILLER_CH];
    for (int k = 0; k < t.np; k++) {
      PairRef r = t.pr[k];
      aff_load<C>(p0[k], parr.base[r.p_arr] + e * parr.stride[r.p_arr] + (size_t)r.p_idx * AFFB(C, Fq<C>));
      aff_load<C>(qs[k], qarr.base[r.q_arr] + e * qarr.stride[r.q_arr] + (size_t)r.q_idx * AFFB(C, Fp2<C>));
      if (r.neg) p0[k].y = neg(p0[k].y);
    }
    Fp12<C> f;
    multi_miller(f, p0, qs, t.np, ts, live, anyfx ? fx : nullptr);
    out[(size_t)ostride * go] = f;  // the task's own cell (slot 0 of 2), or densely packed (batched verifier)
  }
}
};

// ---- pair-cooperative twin (multi_miller_pair): two lanes per (equation, task), one accumulator each ----------------
// Exchange policies: how a lane hands its tangent / chord line (real form: 5 L dwords) to its partner lane ^ 1 (put /
// get, see multi_miller_pair).
//  * PairLds: a 16-byte-interleaved LDS slot per lane, [ceil(5 L / 4)][64] x int4 (conflict-free ds_write_b128 /
//    ds_read_b128, 18 + 18 instructions for BLS12-381, 18 KB; 21 + 21 and 21 KB with general lines); the block is ONE wave, so program order is LDS order and the barriers below
//    are compiler fences; the partner's line is fetched only after the lane's own line product;
//  * PairDpp: one v_mov_b32 with quad_perm [1,0,3,2] per dword at put(), no memory at all.
// Measured at 2^16 (one box, alternating).  First shape of the round loop: DPP 157.1-158.9 ms, LDS 161.3-161.6 ms.
// Final shape (the products of a round in one lambda, gs_pairing.cuh): LDS **147.5-147.7 ms**, DPP 154.6-156.0 ms on
// BLS12-381 (a line parked in LDS frees 84 registers across the lane's own product); BN254 100.5 (DPP) against
// 101.3 ms (LDS).  The planner takes LDS on BLS12-381 and DPP on BN254 (profiles/r3/ab_exchange.txt).
// (a line is LINE_WORDS dwords: 5 L in the real form -- l0, lx in Fp2, ly in Fq --, 6 L under GS_LINES_GENERAL)
template <class C> constexpr int line_words() { return (int)(sizeof(Line<C>) / sizeof(int32_t)); }
template <class C> GS_HD int32_t& line_word(Line<C>& l, int i) {
  constexpr int L = C::L;
  const int c = i / L, j = i % L;
#if defined(GS_LINES_GENERAL)
  return c == 0 ? l.l0.c0.v[j] : c == 1 ? l.l0.c1.v[j] : c == 2 ? l.lx.c0.v[j] : c == 3 ? l.lx.c1.v[j]
         : c == 4 ? l.ly.c0.v[j] : l.ly.c1.v[j];
#else
  return c == 0 ? l.l0.c0.v[j] : c == 1 ? l.l0.c1.v[j] : c == 2 ? l.lx.c0.v[j] : c == 3 ? l.lx.c1.v[j] : l.ly.v[j];
#endif
}
template <class C> struct PairLds {
  int4* slots;  // [W][64]
  int lane;
  // 16-byte words of a slot: 5 L = 70 / 50 dwords are 17.5 / 12.5 of them, the last word is half padding (written as 0,
  // not read back).  Lane l's q-th word sits at int4 index 64 q + l: a ds_write_b128 / ds_read_b128 of the wave touches 64
  // consecutive 16-byte words whatever W is, conflict-free as before; lane ^ 1 only swaps neighbours inside that run.
  static constexpr int NW = line_words<C>();
  static constexpr int W = (NW + 3) / 4;
  __device__ __forceinline__ void put(const Line<C>& mine) const {
    Line<C> m = mine;
    __syncthreads();  // (the partner has read the previous line: one wave per block, this only orders the compiler)
#pragma unroll
    for (int q = 0; q < W; q++) {
      int w[4];
#pragma unroll
      for (int e = 0; e < 4; e++) w[e] = 4 * q + e < NW ? line_word(m, 4 * q + e < NW ? 4 * q + e : 0) : 0;
      slots[q * 64 + lane] = make_int4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
  }
  __device__ __forceinline__ Line<C> get() const {
    Line<C> r;
#pragma unroll
    for (int q = 0; q < W; q++) {
      int4 v = slots[q * 64 + (lane ^ 1)];
      const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (4 * q + e < NW) line_word(r, 4 * q + e) = w[e];
    }
    return r;
  }
};
template <class C> struct PairDpp {
  Line<C> got;  // the exchange happens at put(): both lines are in registers from then on
  __device__ __forceinline__ void put(const Line<C>& mine) {
    Line<C> m = mine;
#pragma unroll
    for (int i = 0; i < line_words<C>(); i++)
      line_word(got, i) = __builtin_amdgcn_mov_dpp(line_word(m, i), 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true);
  }
  __device__ __forceinline__ Line<C> get() const { return got; }
};
// Lanes are pair-major inside task-major: lane g works on component g & 1 of pair g >> 1 = (task, equation); a wave is
// 32 equations of one task.  Same task tables and the same output layout as the twin kernel (out[2 go + a]); the
// stepping triples of a task come first in its list (chunk_tasks), the table-reading ones after them.
template <class C, bool DPP>
struct k_miller_pair {
  static __device__ __forceinline__ void run(size_t g, size_t total, int ntask, const MillerTask* tasks, ArrTab parr,
                                                    ArrTab qarr, Fp12<C>* out, const Line<C>* ltab) {
  __shared__ int4 xslots[DPP ? 1 : PairLds<C>::W * 64];
  if (g >= total) return;  // total is even: a pair leaves together
  const int a = (int)(g & 1);
  const size_t gp = g >> 1, N = total / (2 * (size_t)ntask);
  const size_t ti = gp / N, e = gp % N;
  const size_t go = e * ntask + ti;
  MillerTask t = tasks[ti];
  constexpr int OWN = (MILLER_CH + 1) / 2;
  Aff<Fq<C>> ps[MILLER_CH];
  Aff<Fp2<C>> qown[OWN];
  Proj2<C> ts[OWN];
  const Line<C>* fx[MILLER_CH];
  int nstep = 0;
  for (int k = 0; k < t.np; k++) {
    fx[k] = (ltab && t.pr[k].q_arr == 2) ? ltab + (size_t)t.pr[k].q_idx * miller_line_count<C>() : nullptr;
    if (!fx[k]) nstep = k + 1;  // (a prefix by construction)
  }
  uint32_t qok = 0;
  for (int k = 0; k < t.np; k++) {
    PairRef r = t.pr[k];
    aff_load<C>(ps[k], parr.base[r.p_arr] + e * parr.stride[r.p_arr] + ((size_t)r.p_idx + a) * AFFB(C, Fq<C>));
    if (r.neg) ps[k].y = neg(ps[k].y);
    // identity test of Q on the boundary words ((0, 0) is the flag, and the Montgomery form of 0 is 0)
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(qarr.base[r.q_arr] + e * qarr.stride[r.q_arr] +
                                                           (size_t)r.q_idx * AFFB(C, Fp2<C>));
    uint32_t any = 0;
    for (int w = 0; w < (int)(AFFB(C, Fp2<C>) / 4); w++) any |= qw[w];
    if (any) qok |= 1u << k;
  }
  const int rounds = (nstep + 1) / 2;
  for (int r = 0; r < rounds; r++) {
    int k = 2 * r + a;
    if (k >= nstep) k = nstep - 1;  // odd count: lane 1 steps a copy of the last point, never consumed
    PairRef pr = t.pr[k];
    aff_load<C>(qown[r], qarr.base[pr.q_arr] + e * qarr.stride[pr.q_arr] + (size_t)pr.q_idx * AFFB(C, Fp2<C>));
  }
  Fp12<C> f;
  if constexpr (DPP) {
    PairDpp<C> x;
    multi_miller_pair(f, a, ps, qown, qok, nstep, (int)t.np, ts, fx, x);
  } else {
    PairLds<C> x{xslots, (int)threadIdx.x};
    multi_miller_pair(f, a, ps, qown, qok, nstep, (int)t.np, ts, fx, x);
  }
  out[2 * go + a] = f;
}
};

// Cell c = 2a + b: product of its Miller partials (CellMap), final exponentiation,
// compare with 1 or the PPE target (verifier.rs:50-53) -> cellok[e*4+c].
template <class C> GS_HD_NOINLINE void cell_product(Fp12<C>& f, const Fp12<C>* mpart, size_t e, int ntask, int c,
                                                    const CellMap& cm) {
  int lo = cm.lo[c], hi = cm.hi[c], a = cm.sub[c];
  f = mpart[2 * (e * ntask + lo) + a];
  for (int i = lo + 1; i < hi; i++) f12_mul(f, f, mpart[2 * (e * ntask + i) + a]);
}
// Large arities: a cell has hundreds of Miller partials.  One lane per (equation, cell, run of K partials) multiplies
// its run; repeated by the host until k_final's own serial product is short (segmented K-ary tree in GT).
// Output layout = cell_product's: out[2 * (e * nt_out + cm_out.lo[c] + run) + 0].
template <class C>
struct k_cell_fold {
  static __device__ __forceinline__ void run(size_t g, size_t total, int runs_max, int ntask_in, CellMap cm_in,
                                                          const Fp12<C>* in, int K, int nt_out, CellMap cm_out,
                                                          Fp12<C>* out) {
  if (g >= total) return;
  int run = (int)(g % runs_max);
  int c = (int)((g / runs_max) & 3);
  size_t e = g / ((size_t)runs_max * 4);
  int lo = cm_in.lo[c] + run * K, hi = lo + K < cm_in.hi[c] ? lo + K : cm_in.hi[c], a = cm_in.sub[c];
  if (lo >= cm_in.hi[c]) return;
  Fp12<C> f = in[2 * (e * ntask_in + lo) + a];
  for (int i = lo + 1; i < hi; i++) f12_mul(f, f, in[2 * (e * ntask_in + i) + a]);
  out[2 * (e * nt_out + cm_out.lo[c] + run)] = f;
}
};

template <class C>
struct k_final {
  static __device__ __forceinline__ void run(size_t g, size_t N, int ntask, CellMap cm, const Fp12<C>* mpart,
                                              const uint8_t* target, uint8_t* cellok) {
  if (g >= N * 4) return;
  size_t e = g >> 2;
  int c = (int)(g & 3);
  Fp12<C> f;
  unsigned long long sf0 = GS_STAMP_T();
  cell_product(f, mpart, e, ntask, c, cm);
  unsigned long long sf1 = GS_STAMP_T();
  Fp12<C> r;
  final_exp(r, f);
  unsigned long long sf2 = GS_STAMP_T();
  bool ok;
  if (c == 3 && target) {
    Fp12<C> t;
    f12_from_boundary<C>(t, reinterpret_cast<const BFq<C>*>(target) + 12 * e);
    ok = f12_eq(r, t);
  } else {
    ok = f12_is_one(r);
  }
  cellok[g] = ok ? 1 : 0;
  GS_STAMP_ADD(6, sf1 - sf0);
  GS_STAMP_ADD(7, sf2 - sf1);
  GS_STAMP_ADD(8, GS_STAMP_T() - sf2);
  GS_STAMP_ADD(9, 1);
}
};

// The same with a 3-lane group per cell (gs_coop.cuh) for batches that cannot fill the chip with one lane per
// final exponentiation.  blockDim.x == 63: one wave = 21 groups; idle groups of the last wave shadow the last cell so
// that every lane reaches the shuffles.
template <class C>
struct k_final_coop {
  static __device__ __forceinline__ void run(size_t gt, size_t N, int ntask, CellMap cm, const Fp12<C>* mpart,
                                                   const uint8_t* target, uint8_t* cellok) {
  int lane = (int)(gt % 63), j = lane % 3;  // 63-thread blocks: gt % 63 is the thread within its block (= wave)
  size_t g = (gt / 63) * 21 + lane / 3;
  bool live = g < N * 4;
  if (!live) g = N * 4 - 1;
  size_t e = g >> 2;
  int c = (int)(g & 3);
  Fp12<C> f;
  cell_product(f, mpart, e, ntask, c, cm);
  Fp12<C> r;
  CoopWave xw{lane - j};
  ExpXCoop<C, CoopWave> ex{j, &xw};
  final_exp_with(r, f, ex);
  bool ok;
  if (c == 3 && target) {
    Fp12<C> t;
    f12_from_boundary<C>(t, reinterpret_cast<const BFq<C>*>(target) + 12 * e);
    ok = f12_eq(r, t);
  } else {
    ok = f12_is_one(r);
  }
  if (live && j == 0) cellok[g] = ok ? 1 : 0;
}
};

struct k_and4 {
  static __device__ __forceinline__ void run(size_t e_in, size_t N, const uint8_t* cellok, uint8_t* ok) {
  size_t e = e_in;
  if (e >= N) return;
  const uint8_t* c = cellok + e * 4;
  ok[e] = (c[0] & c[1] & c[2] & c[3]) ? 1 : 0;
}
};

// ---- equation evaluation (gs_eval_* / gs_check_witness_*): the left-hand sides of statement.rs:17-21 ---------------
// Fr preparation, one lane per equation.  The Gamma term is folded into the scalars of the OTHER side so that it costs
// no scalar multiplication of its own:
//   PPE      Gamma -> canonical (GC); the fold is W_j = A_j + sum_i Gamma_ij X_i in G1, on the Straus lanes
//   MSMEG1   y_j -> canonical (YC),  c_i = b_i + sum_j Gamma_ij y_j (BC):  value = sum_j y_j A_j + sum_i c_i X_i
//   MSMEG2   x_i -> canonical (XC),  d_j = a_j + sum_i x_i Gamma_ij (AC):  value = sum_i x_i B_i + sum_j d_j Y_j
//   QuadEqu  the value itself, sum_j a_j y_j + sum_i x_i c_i, a canonical Montgomery Fr: written to out[e], or (ok
//            non-null) compared limb by limb with tq[e] -- a target with non-canonical limbs never matches
// shared_vars: a Statement -- ONE copy of the variables xs / ys for all equations.  folded (QuadEqu, large arities): the
// c_i are in the pool already, in Montgomery form (k_prep_eval_wide).
template <class C>
struct k_prep_eval {
  static __device__ __forceinline__ void run(size_t e_in, size_t N, int ty, int m, int n, const Fr<C>* G, const Fr<C>* xs,
                                              const Fr<C>* ys, const Fr<C>* as, const Fr<C>* bs, PoolMap pm, Fr<C>* pool,
                                              int shared_vars, int folded, const Fr<C>* tq, Fr<C>* out, uint8_t* ok) {
  size_t e = e_in;
  if (e >= N) return;
  typedef Fr<C> S_;
  const size_t ev = shared_vars ? 0 : e;
  if (G) G += e * (size_t)m * n;
  if (xs) xs += ev * m;
  if (ys) ys += ev * n;
  if (as) as += e * n;
  if (bs) bs += e * m;
  S_* P = pool + e * pm.total;
  if (ty == 0) {
    for (int i = 0; i < m * n; i++) P[pm.GC + i] = from_mont(G[i]);
    return;
  }
  if (ty == 1) {
    for (int j = 0; j < n; j++) P[pm.YC + j] = from_mont(ys[j]);
    for (int i = 0; i < m; i++) {
      S_ ci = bs[i];
      for (int j = 0; j < n; j++) ci = add(ci, mul(G[i * n + j], ys[j]));
      P[pm.BC + i] = from_mont(ci);
    }
    return;
  }
  if (ty == 2) {
    for (int i = 0; i < m; i++) P[pm.XC + i] = from_mont(xs[i]);
    for (int j = 0; j < n; j++) {
      S_ dj = as[j];
      for (int i = 0; i < m; i++) dj = add(dj, mul(xs[i], G[i * n + j]));
      P[pm.AC + j] = from_mont(dj);
    }
    return;
  }
  S_ v = fzero<FrM<C>>();
  for (int j = 0; j < n; j++) v = add(v, mul(as[j], ys[j]));
  for (int i = 0; i < m; i++) {
    S_ ci;
    if (folded) {
      ci = P[pm.BC + i];
    } else {
      ci = bs[i];
      for (int j = 0; j < n; j++) ci = add(ci, mul(G[i * n + j], ys[j]));
    }
    v = add(v, mul(xs[i], ci));
  }
  if (ok)
    ok[e] = eq(v, tq[e]) ? 1 : 0;
  else
    out[e] = v;
}
};
// The same for large arities (wide_prep): one lane per OUTPUT SCALAR, W per equation -- n + m for the two MSME types
// (the canonical variables, then the folded c_i / d_j), m for QuadEqu (the c_i, kept in Montgomery form for
// k_prep_eval's final sum).  PPE needs only Gamma in canonical form: k_fr_canonical.
template <class C>
struct k_prep_eval_wide {
  static __device__ __forceinline__ void run(size_t g, size_t total, int W, int ty, int m, int n, const Fr<C>* G,
                                              const Fr<C>* xs, const Fr<C>* ys, const Fr<C>* as, const Fr<C>* bs,
                                              PoolMap pm, Fr<C>* pool, int shared_vars) {
  if (g >= total) return;
  typedef Fr<C> S_;
  size_t e = g / W;
  int w = (int)(g % W);
  const size_t ev = shared_vars ? 0 : e;
  G += e * (size_t)m * n;
  if (xs) xs += ev * m;
  if (ys) ys += ev * n;
  if (as) as += e * n;
  if (bs) bs += e * m;
  S_* P = pool + e * pm.total;
  if (ty == 2) {
    if (w < m) {
      P[pm.XC + w] = from_mont(xs[w]);
      return;
    }
    int j = w - m;
    S_ dj = as[j];
    for (int i = 0; i < m; i++) dj = add(dj, mul(xs[i], G[i * n + j]));
    P[pm.AC + j] = from_mont(dj);
    return;
  }
  if (ty == 1 && w < n) {
    P[pm.YC + w] = from_mont(ys[w]);
    return;
  }
  int i = ty == 1 ? w - n : w;
  S_ ci = bs[i];
  for (int j = 0; j < n; j++) ci = add(ci, mul(G[i * n + j], ys[j]));
  P[pm.BC + i] = ty == 1 ? from_mont(ci) : ci;
}
};

// k_red for outputs of ONE point each (the evaluated MSME value, the W_j of a PPE): up to K consecutive outputs per lane
// behind one shared inversion; output t.out_idx of array t.out_arr is a point index.  Only the run [b0, e0) of a
// RedTask is read.
template <class C, class F>
struct k_red_pt {
  static __device__ __forceinline__ void run(size_t g, size_t total, int ntask, const RedTask* tasks, const Jac<F>* part,
                                              int nslots, OutTab outs, int K) {
  if (g >= total) return;
  const int nl = (ntask + K - 1) / K;  // lanes per equation
  size_t e = g / nl;
  int t0 = (int)(g % nl) * K, nt = ntask - t0 < K ? ntask - t0 : K;
  const Jac<F>* P = part + e * nslots;
  Jac<F> s[RED_K];
  F pre[RED_K];  // pre[i] = z_0 ... z_(i-1) (identities count as 1)
  F acc = one_of<F>();
  for (int k = 0; k < nt; k++) {
    RedTask t = tasks[t0 + k];
    Jac<F> s0 = P[t.b0];
    for (uint32_t i = t.b0 + 1; i < t.e0; i++) jac_add(s0, s0, P[i]);
    s[k] = s0;
    pre[k] = acc;
    if (!is_zero_limbs(s0.z)) acc = mul(acc, s0.z);
  }
  F suf = inv(acc);  // 1 / (z_0 ... z_(nt - 1))
  for (int i = nt - 1; i >= 0; i--) {
    RedTask t = tasks[t0 + i];
    Aff<F> a;
    F zi = mul(suf, pre[i]);  // 1 / z_i
    if (!is_zero_limbs(s[i].z)) suf = mul(suf, s[i].z);
    jac_to_aff_zinv(a, s[i], zi);  // (identity -> (0, 0), zi unused)
    aff_store<C>(outs.base[t.out_arr] + e * outs.stride[t.out_arr] + (size_t)t.out_idx * AFFB(C, F), a);
  }
}
};

// The end of a PPE evaluation: FE(product of the equation's Miller partials) is WRITTEN in boundary form to out[e], or
// (ok non-null) compared with target[e].  The comparison is on the boundary limbs themselves: the value's are canonical,
// so a target with non-canonical limbs never matches (f12_from_boundary + f12_eq would reduce it first).
template <class C>
GS_HD_NOINLINE void eval_gt_finish(const Fp12<C>& r, size_t e, const uint8_t* target, uint8_t* out, uint8_t* ok) {
  if (!ok) {
    f12_to_boundary<C>(reinterpret_cast<BFq<C>*>(out) + 12 * e, r);
    return;
  }
  BFq<C> x[12];
  f12_to_boundary<C>(x, r);
  const BFq<C>* t = reinterpret_cast<const BFq<C>*>(target) + 12 * e;
  uint32_t o = 0;
  for (int i = 0; i < 12; i++)
    for (int j = 0; j < C::N; j++) o |= x[i].w[j] ^ t[i].w[j];
  ok[e] = o == 0 ? 1 : 0;
}
// partials of equation e: mpart[ostride * (e * ntask + i)], i < ntask (ostride 2: the layout k_cell_fold leaves)
template <class C>
GS_HD_NOINLINE void eval_product(Fp12<C>& f, const Fp12<C>* mpart, size_t e, int ntask, int ostride) {
  f = mpart[(size_t)ostride * (e * ntask)];
  for (int i = 1; i < ntask; i++) f12_mul(f, f, mpart[(size_t)ostride * (e * ntask + i)]);
}
// ONE cell per equation; the body of k_final / k_final_coop otherwise
template <class C>
struct k_final_eval {
  static __device__ __forceinline__ void run(size_t e_in, size_t N, int ntask, int ostride, const Fp12<C>* mpart,
                                              const uint8_t* target, uint8_t* out, uint8_t* ok) {
  size_t e = e_in;
  if (e >= N) return;
  Fp12<C> f;
  eval_product(f, mpart, e, ntask, ostride);
  Fp12<C> r;
  final_exp(r, f);
  eval_gt_finish<C>(r, e, target, out, ok);
}
};
// 3-lane group per equation (blockDim.x == 63: one wave = 21 groups; idle groups of the last wave shadow the last equation
// so that every lane reaches the shuffles)
template <class C>
struct k_final_eval_coop {
  static __device__ __forceinline__ void run(size_t gt, size_t N, int ntask, int ostride, const Fp12<C>* mpart,
                                              const uint8_t* target, uint8_t* out, uint8_t* ok) {
  int lane = (int)(gt % 63), j = lane % 3;
  size_t e = (gt / 63) * 21 + lane / 3;
  bool live = e < N;
  if (!live) e = N - 1;
  Fp12<C> f;
  eval_product(f, mpart, e, ntask, ostride);
  Fp12<C> r;
  CoopWave xw{lane - j};
  ExpXCoop<C, CoopWave> ex{j, &xw};
  final_exp_with(r, f, ex);
  if (live && j == 0) eval_gt_finish<C>(r, e, target, out, ok);
}
};
// ok[e] = (the evaluated point e == target e) on their boundary words: the value is normalised affine with canonical
// limbs (the identity all-zero), so equality as elements is equality of words and a non-canonical target never matches
struct k_eval_cmp {
  static __device__ __forceinline__ void run(size_t e_in, size_t N, int words, const uint32_t* val, const uint32_t* tgt,
                                              uint8_t* ok) {
  size_t e = e_in;
  if (e >= N) return;
  uint32_t o = 0;
  for (int w = 0; w < words; w++) o |= val[e * words + w] ^ tgt[e * words + w];
  ok[e] = o == 0 ? 1 : 0;
}
};

// E::multi_pairing per row: k pairs -> Miller product -> final exponentiation
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_multi_pairing(size_t n, int k, const uint8_t* P, const uint8_t* Q,
                                                      uint8_t* out) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  Aff<Fq<C>> ps[MILLER_CH];
  Aff<Fp2<C>> qs[MILLER_CH];
  Proj2<C> ts[MILLER_CH];
  bool live[MILLER_CH];
  Fp12<C> acc, f;
  f12_one(acc);
  for (int b = 0; b < k; b += MILLER_CH) {
    int np = k - b < MILLER_CH ? k - b : MILLER_CH;
    for (int i = 0; i < np; i++) {
      aff_load<C>(ps[i], P + (g * k + b + i) * AFFB(C, Fq<C>));
      aff_load<C>(qs[i], Q + (g * k + b + i) * AFFB(C, Fp2<C>));
    }
    multi_miller(f, ps, qs, np, ts, live);
    f12_mul(acc, acc, f);
  }
  final_exp(f, acc);
  f12_to_boundary<C>(reinterpret_cast<BFq<C>*>(out) + 12 * g, f);
}

// out[i] = base^(k[i]) for base in GT (cyclotomic squarings are valid)
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_gt_pow(size_t n, const uint8_t* base, const Fr<C>* k, uint8_t* out) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  Fr<C> s = from_mont(k[g]);
  Fp12<C> b, acc;
  f12_from_boundary<C>(b, reinterpret_cast<const BFq<C>*>(base));
  f12_one(acc);
  bool started = false;
  int since = 0;
  for (int i = FrM<C>::BITS - 1; i >= 0; i--) {
    if (started) {
      f12_cyclo_sqr(acc, acc);
      since++;
    }
    if (get_bit(s, i)) {
      if (started)
        f12_mul(acc, acc, b);
      else
        acc = b;
      started = true;
      since = 0;
    } else if (since == 3) {
      f12_vreduce(acc);
      since = 0;
    }
  }
  f12_to_boundary<C>(reinterpret_cast<BFq<C>*>(out) + 12 * g, acc);
}

// ---- batched (random-linear-combination) verifier: tree product + one final exponentiation ----
// out[i] = product of in[i*K .. min((i+1)*K, n_in))
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_gt_prod(size_t n_in, const Fp12<C>* in, size_t n_out, Fp12<C>* out,
                                                        int K) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_out) return;
  size_t lo = g * (size_t)K, hi = lo + K < n_in ? lo + K : n_in;
  Fp12<C> acc = in[lo];
  for (size_t i = lo + 1; i < hi; i++) f12_mul(acc, acc, in[i]);
  out[g] = acc;
}
// internal <-> boundary copies of GT arrays (accumulators cross the API in boundary form)
template <class C> __global__ void __launch_bounds__(64, GS_WPE) k_gt_export(size_t n, const Fp12<C>* in, uint8_t* out) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  f12_to_boundary<C>(reinterpret_cast<BFq<C>*>(out) + 12 * g, in[g]);
}
template <class C> __global__ void __launch_bounds__(64, GS_WPE) k_gt_import(size_t n, const uint8_t* in, Fp12<C>* out) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  Fp12<C> t;
  f12_from_boundary<C>(t, reinterpret_cast<const BFq<C>*>(in) + 12 * g);
  out[g] = t;
}
// acc[0] = Miller-side accumulator, acc[1] = target-side accumulator: ok = (FE(acc[0]) == acc[1])
// launched with ONE block of 3 lanes: a single 3-lane cooperative final exponentiation
template <class C> __global__ void k_fe_eq(const Fp12<C>* acc, uint8_t* ok) {
  int j = (int)threadIdx.x;
  Fp12<C> r;
  CoopWave xw{0};
  ExpXCoop<C, CoopWave> ex{j, &xw};
  final_exp_with(r, acc[0], ex);
  bool same = f12_eq(r, acc[1]);
  if (j == 0) ok[0] = same ? 1 : 0;
}
template <class C> __global__ void k_gt_set_one(Fp12<C>* p) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Fp12<C> o;
  f12_one(o);
  p[0] = o;
}

// ---- statement-batched verifier (gs_verify_statements_rlc): the unit of every array is a STATEMENT of E equations ----
// Fr preparation.  Output scalar o of statement s (canonical, pool of pm.total scalars per statement):
//   [0, 4E)        RH[4e + c]                 = rho[s][e][c]
//   then 4mn       GC[(c m + i) n + j]        = sum_e rho_e,c Gamma_e,ij
//   then 4n  (as)  AR[4j + c]                 = sum_e rho_e,c a_ej          (scalar constants on the X side)
//   then 4m  (bs)  BC[4i + c]                 = sum_e rho_e,c b_ei          (scalar constants on the Y side)
//   then 4   (tq)  NR[c]                      = - sum_e rho_e,c t_e         (QuadEqu targets)
// every sum is E products: a lane that owns ONE output never walks more than E terms.
template <class C>
__device__ __forceinline__ void stmt_prep_out(size_t s, int o, int E, int m, int n, const Fr<C>* G, const Fr<C>* as,
                                              const Fr<C>* bs, const Fr<C>* tq, const uint64_t* rho, const PoolMap& pm,
                                              Fr<C>* P) {
  const uint64_t* rs = rho + s * (size_t)E * 4;
  auto rho_fr = [&](int idx) {
    Fr<C> r = fzero<FrM<C>>();
    uint64_t v = rs[idx];
    r.v[0] = (uint32_t)v;
    r.v[1] = (uint32_t)(v >> 32);
    return r;  // canonical (rho < 2^64 < r)
  };
  if (o < 4 * E) {
    P[pm.RH + o] = rho_fr(o);
    return;
  }
  o -= 4 * E;
  const int mn = m * n;
  const Fr<C>* src;
  int stride, c, dst;
  bool negate = false;
  if (o < 4 * mn) {
    c = o / mn;
    src = G + s * (size_t)E * mn + (o % mn);
    stride = mn;
    dst = pm.GC + o;
  } else {
    o -= 4 * mn;
    if (as && o < 4 * n) {
      c = o & 3;
      src = as + s * (size_t)E * n + (o >> 2);
      stride = n;
      dst = pm.AR + o;
    } else {
      if (as) o -= 4 * n;
      if (bs && o < 4 * m) {
        c = o & 3;
        src = bs + s * (size_t)E * m + (o >> 2);
        stride = m;
        dst = pm.BC + o;
      } else {
        if (bs) o -= 4 * m;
        c = o;
        src = tq + s * (size_t)E;
        stride = 1;
        dst = pm.NR + o;
        negate = true;
      }
    }
  }
  Fr<C> acc = fzero<FrM<C>>();
  for (int e = 0; e < E; e++) acc = add(acc, mul(src[(size_t)e * stride], to_mont(rho_fr(4 * e + c))));
  if (negate) acc = neg(acc);
  P[dst] = from_mont(acc);
}
// per = 1: one lane per statement walks its nout outputs (small statements); per = nout: one lane per output scalar
template <class C>
__global__ void __launch_bounds__(64, GS_WPE)
    k_prep_verify_stmt_rlc(size_t S, int E, int m, int n, int nout, int per, const Fr<C>* G, const Fr<C>* as,
                           const Fr<C>* bs, const Fr<C>* tq, const uint64_t* rho, PoolMap pm, Fr<C>* pool) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= S * (size_t)per) return;
  size_t s = g / per;
  Fr<C>* P = pool + s * pm.total;
  if (per == 1) {
    for (int o = 0; o < nout; o++) stmt_prep_out<C>(s, o, E, m, n, G, as, bs, tq, rho, pm, P);
  } else {
    stmt_prep_out<C>(s, (int)(g % per), E, m, n, G, as, bs, tq, rho, pm, P);
  }
}

// segmented product: S segments of len_in elements each -> S segments of len_out = ceil(len_in / K) products of runs
// of K (the host repeats it until len_out = 1, as gt_product does for one segment)
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_gt_prod_seg(size_t S, size_t len_in, const Fp12<C>* in, size_t len_out,
                                                            Fp12<C>* out, int K) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= S * len_out) return;
  size_t s = g / len_out, r = g % len_out;
  size_t lo = r * (size_t)K, hi = lo + K < len_in ? lo + K : len_in;
  const Fp12<C>* p = in + s * len_in;
  Fp12<C> acc = p[lo];
  for (size_t i = lo + 1; i < hi; i++) f12_mul(acc, acc, p[i]);
  out[s * len_out + r] = acc;
}

// One statement: product of its ntask Miller partials (the un-exponentiated accumulator), final exponentiation,
// comparison with the statement's target product (tprod; null = one).  Writes the verdict and the boundary-form pair
// (acc[s][0] = Miller product, acc[s][1] = target product) that gs_gt_finalize takes.
template <class C> __device__ __forceinline__ void miller_product(Fp12<C>& f, const Fp12<C>* mpart, size_t s, int ntask) {
  const Fp12<C>* p = mpart + s * (size_t)ntask;
  f = p[0];
  for (int i = 1; i < ntask; i++) f12_mul(f, f, p[i]);
}
template <class C>
__device__ __forceinline__ void stmt_product(Fp12<C>& f, Fp12<C>& t, const Fp12<C>* mpart, const Fp12<C>* tprod, size_t s,
                                             int ntask) {
  miller_product(f, mpart, s, ntask);
  if (tprod)
    t = tprod[s];
  else
    f12_one(t);
}
template <class C>
struct k_stmt_final {
  static __device__ __forceinline__ void run(size_t s, size_t S, int ntask, const Fp12<C>* mpart, const Fp12<C>* tprod,
                                             uint8_t* acc, uint8_t* ok) {
  if (s >= S) return;
  Fp12<C> f, t, r;
  stmt_product(f, t, mpart, tprod, s, ntask);
  BFq<C>* a = reinterpret_cast<BFq<C>*>(acc) + 24 * s;
  f12_to_boundary<C>(a, f);
  f12_to_boundary<C>(a + 12, t);
  final_exp(r, f);
  ok[s] = f12_eq(r, t) ? 1 : 0;
}
};
// The same with a 3-lane group per statement (gs_coop.cuh; blockDim.x == 63: 21 groups per wave, idle groups of the
// last wave shadow the last statement so that every lane reaches the shuffles)
template <class C>
struct k_stmt_final_coop {
  static __device__ __forceinline__ void run(size_t gt, size_t S, int ntask, const Fp12<C>* mpart, const Fp12<C>* tprod,
                                             uint8_t* acc, uint8_t* ok) {
  int lane = (int)(gt % 63), j = lane % 3;
  size_t s = (gt / 63) * 21 + lane / 3;
  bool live = s < S;
  if (!live) s = S - 1;
  Fp12<C> f, t, r;
  stmt_product(f, t, mpart, tprod, s, ntask);
  if (live && j == 0) {
    BFq<C>* a = reinterpret_cast<BFq<C>*>(acc) + 24 * s;
    f12_to_boundary<C>(a, f);
    f12_to_boundary<C>(a + 12, t);
  }
  CoopWave xw{lane - j};
  ExpXCoop<C, CoopWave> ex{j, &xw};
  final_exp_with(r, f, ex);
  bool same = f12_eq(r, t);
  if (live && j == 0) ok[s] = same ? 1 : 0;
}
};

// ---- fault localisation of the batched verifier (gs_verify_batch_rlc_locate): K-ary product tree, kept ----------------
// Leaf e = (f_e, t_e): f_e the product of equation e's ntask Miller partials, t_e = k_rlc_tpow's power (PPE; one
// otherwise, not stored).  Node (l, i) = product of nodes (l-1, i K .. i K + K - 1).  All levels live in one buffer per
// side, level after level.  A node passes iff FE(f) == t; the descent checks the root and every child of a failing node.
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_rlc_leaf(size_t N, int ntask, const Fp12<C>* mpart, Fp12<C>* f0) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  Fp12<C> f;
  miller_product(f, mpart, e, ntask);
  f0[e] = f;
}
// one level up, both sides in one launch: lanes [0, n_out) fold fin, lanes [half, half + n_out) fold tin (tin null: the
// launch ends at n_out); half = n_out rounded up to whole waves, so no wave straddles the sides
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_rlc_tree(size_t n_in, const Fp12<C>* fin, const Fp12<C>* tin, size_t n_out,
                                                         Fp12<C>* fout, Fp12<C>* tout, int K) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t half = (n_out + 63) / 64 * 64;
  const bool ts = g >= half;
  if (ts) g -= half;
  if (g >= n_out || (ts && !tin)) return;
  const Fp12<C>* in = ts ? tin : fin;
  size_t lo = g * (size_t)K, hi = lo + K < n_in ? lo + K : n_in;
  Fp12<C> acc = in[lo];
  for (size_t i = lo + 1; i < hi; i++) f12_mul(acc, acc, in[i]);
  (ts ? tout : fout)[g] = acc;
}
// One level of the descent.  Item g = (failing parent fr_in[g / fan], child g % fan); the child is node
// fr_in[g / fan] * fan + g % fan of this level if that is < n_child (the last parent of a level may have fewer children).
// The launch covers the whole level; *cnt_in (device memory) says how much of it there is to do.
struct LocateLevel {
  const uint32_t* fr_in;   // failing nodes one level up (order free)
  const uint32_t* cnt_in;  // how many
  uint32_t* fr_out;        // failing nodes of this level are appended here ...
  uint32_t* cnt_out;       // ... and counted here (both unused at level 0)
  uint32_t n_child;        // nodes of this level
  int fan;                 // children per parent: K, or 1 for the root under its virtual parent
  uint8_t* ok;             // level 0 only: ok[e] = 0 for a failing leaf
  uint32_t* info;          // [0] += failing leaves, [1] += node checks
};
// the wave's bookkeeping: one ballot per flag, one atomic per counter and wave (lane 0; every lane of the wave is here)
__device__ __forceinline__ void locate_commit(const LocateLevel& L, int lane, bool checked, bool bad, uint32_t node) {
  const unsigned long long mc = __ballot(checked), mb = __ballot(bad);
  uint32_t base = 0;
  if (lane == 0) {
    if (mc) atomicAdd(L.info + 1, (uint32_t)__popcll(mc));
    if (mb) {
      if (L.ok)
        atomicAdd(L.info, (uint32_t)__popcll(mb));
      else
        base = atomicAdd(L.cnt_out, (uint32_t)__popcll(mb));
    }
  }
  if (L.ok) {
    if (bad) L.ok[node] = 0;
    return;
  }
  base = (uint32_t)__shfl((int)base, 0, 64);
  if (bad) L.fr_out[base + (uint32_t)__popcll(mb & ((1ull << lane) - 1))] = node;
}
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_rlc_locate(LocateLevel L, const Fp12<C>* F, const Fp12<C>* T) {
  const int lane = (int)threadIdx.x;
  const size_t g0 = (size_t)blockIdx.x * blockDim.x, g = g0 + lane;
  const size_t items = (size_t)*L.cnt_in * (size_t)L.fan;
  if (g0 >= items) return;  // a whole wave beyond the frontier
  bool live = g < items;
  size_t node = 0;
  if (live) {
    node = (size_t)L.fr_in[g / L.fan] * (size_t)L.fan + g % L.fan;
    live = node < L.n_child;
  }
  bool bad = false;
  if (live) {
    Fp12<C> f = F[node], t, r;
    if (T)
      t = T[node];
    else
      f12_one(t);
    final_exp(r, f);
    bad = !f12_eq(r, t);
  }
  locate_commit(L, lane, live, bad, (uint32_t)node);
}
// The same with a 3-lane group per item (gs_coop.cuh; blockDim.x == 63: 21 groups per wave).  Idle groups of a live wave
// shadow child 0 of the first frontier node (it always exists) so that every lane reaches the shuffles.
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_rlc_locate_coop(LocateLevel L, const Fp12<C>* F, const Fp12<C>* T) {
  const int lane = (int)threadIdx.x, j = lane % 3;
  const size_t g0 = (size_t)blockIdx.x * 21, g = g0 + lane / 3;
  const size_t items = (size_t)*L.cnt_in * (size_t)L.fan;
  if (g0 >= items) return;  // a whole wave beyond the frontier
  bool live = g < items;
  size_t node = 0;
  if (live) {
    node = (size_t)L.fr_in[g / L.fan] * (size_t)L.fan + g % L.fan;
    live = node < L.n_child;
  }
  if (!live) node = (size_t)L.fr_in[0] * (size_t)L.fan;
  Fp12<C> f = F[node], t, r;
  if (T)
    t = T[node];
  else
    f12_one(t);
  CoopWave xw{lane - j};
  ExpXCoop<C, CoopWave> ex{j, &xw};
  final_exp_with(r, f, ex);
  const bool same = f12_eq(r, t);
  const bool mine = live && j == 0;
  locate_commit(L, lane, mine, mine && !same, (uint32_t)node);
}

// --------------------------------------------------------------------------
// wire format (gs_wire.cuh): arrays of elements, one lane per element
// --------------------------------------------------------------------------
template <class C, class F> constexpr size_t wire_point_bytes(bool compressed) {
  return (size_t)(compressed ? 1 : 2) * NCoord<F>::V * C::N * 4;
}
template <class C, class F>
__global__ void __launch_bounds__(64, GS_WPE) k_wire_enc_pts(size_t n, const uint8_t* pts, int compressed, uint8_t* out) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  Aff<F> p;
  aff_load<C>(p, pts + g * AFFB(C, F));
  wire_encode_point<C, F>(out + g * wire_point_bytes<C, F>(compressed != 0), p, compressed != 0);
}
template <class C, class F>
__global__ void __launch_bounds__(64, GS_WPE) k_wire_dec_pts(size_t n, const uint8_t* in, int compressed, int validate,
                                                     uint8_t* pts, uint8_t* ok) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  Aff<F> p;
  bool good = wire_decode_point<C, F>(p, in + g * wire_point_bytes<C, F>(compressed != 0), compressed != 0, validate != 0);
  aff_store<C>(pts + g * AFFB(C, F), p);
  ok[g] = good ? 1 : 0;
}
// In-memory points (boundary limbs, include/gs_amd.h) through the checks the wire decoder applies to decoded ones:
// canonical coordinates (every Montgomery word string < p), the identity flag (0, 0), on the curve, and in the r-torsion
// (the endomorphism tests of gs_wire.cuh).  The reference's plain double-and-add takes ANY curve point
// (data_structures.rs:336-342); the GLV / psi-GLS scalar multiplications here are only defined on the r-torsion, so a
// caller that did not get its points from a validating decoder asks this first (or turns the endomorphisms off).
template <class C, class F>
__global__ void __launch_bounds__(64, GS_WPE) k_validate_pts(size_t n, const uint8_t* pts, uint8_t* ok) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  constexpr int NW = (int)(AFFB(C, F) / (4 * C::N));  // Fq words strings per point: 2 (G1) or 4 (G2)
  const uint32_t* w = reinterpret_cast<const uint32_t*>(pts + g * AFFB(C, F));
  bool canon = true, zero = true;
  for (int k = 0; k < NW; k++) {
    uint32_t t[C::N];
    for (int i = 0; i < C::N; i++) t[i] = w[k * C::N + i];
    canon = canon && words_lt_p<C>(t);
    zero = zero && words_zero<C::N>(t);
  }
  bool good = canon;
  if (canon && !zero) {
    Aff<F> p;
    aff_load<C>(p, pts + g * AFFB(C, F));
    good = eq(sqr(p.y), curve_rhs<C>(p.x)) && in_prime_subgroup<C>(p);
  }
  ok[g] = good ? 1 : 0;
}
// Fq arrays (GT = 12 per element): dir 0 boundary -> canonical little-endian bytes, dir 1 back (ok = canonical)
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_wire_fq(size_t n, int dir, const uint8_t* in, uint8_t* out, uint8_t* ok) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  constexpr int B = C::N * 4;
  uint32_t w[C::N];
  if (dir == 0) {
    BFq<C> b = reinterpret_cast<const BFq<C>*>(in)[g];
    fq_to_canonical<C>(w, fq_from_boundary<C>(b.w));
    for (int i = 0; i < B; i++) out[g * B + i] = (uint8_t)(w[i >> 2] >> ((i & 3) * 8));
  } else {
    for (int i = 0; i < C::N; i++) w[i] = 0;
    for (int i = 0; i < B; i++) w[i >> 2] |= (uint32_t)in[g * B + i] << ((i & 3) * 8);
    bool canon = words_lt_p<C>(w);
    BFq<C> b;
    if (!canon)
      for (int i = 0; i < C::N; i++) w[i] = 0;
    fq_to_boundary<C>(b.w, fq_from_canonical<C>(w));
    reinterpret_cast<BFq<C>*>(out)[g] = b;
    ok[g] = canon ? 1 : 0;
  }
}
template <class C>
__global__ void __launch_bounds__(64, GS_WPE) k_wire_fr(size_t n, int dir, const uint8_t* in, uint8_t* out, uint8_t* ok) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  constexpr int NW = FrM<C>::N, B = NW * 4;
  if (dir == 0) {
    Fr<C> k = from_mont(reinterpret_cast<const Fr<C>*>(in)[g]);
    for (int i = 0; i < B; i++) out[g * B + i] = (uint8_t)(k.v[i >> 2] >> ((i & 3) * 8));
  } else {
    Fr<C> k;
    uint32_t r[NW];
    for (int i = 0; i < NW; i++) {
      k.v[i] = 0;
      r[i] = C::R_WORDS[i];
    }
    for (int i = 0; i < B; i++) k.v[i >> 2] |= (uint32_t)in[g * B + i] << ((i & 3) * 8);
    bool canon = words_gt<NW>(r, k.v);
    if (!canon)
      for (int i = 0; i < NW; i++) k.v[i] = 0;
    reinterpret_cast<Fr<C>*>(out)[g] = to_mont(k);
    ok[g] = canon ? 1 : 0;
  }
}
template <class C> __global__ void __launch_bounds__(64, GS_WPE) k_wire_gt_check(size_t n, const uint8_t* gt, uint8_t* ok) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  Fp12<C> f;
  f12_from_boundary<C>(f, reinterpret_cast<const BFq<C>*>(gt) + 12 * g);
  ok[g] = (ok[g] && f12_in_torsion(f)) ? 1 : 0;
}

}  // namespace gs
