// gs_layout.h -- the byte sizes of a batch's arrays, once.
//
// Every prove / verify / rerandomize entry point of include/gs_amd.h moves the same fourteen named arrays; how many
// bytes each holds follows from the curve (bytes of an Fq), the equation type, the batch size N, the shape (m, n) and
// whether the variables are a Statement's (`shared`: ONE copy of X, Y, R, S and of the commitments for all N
// equations).  The host code that stages, shards or checks those arrays takes its sizes from here and nowhere else
// (the Python binding keeps its own copy of this table, Engine._sizes; tests/test_layout.py holds the two against
// each other).  Plain C++17, no HIP: the table is also compiled by itself on the host.
#ifndef GS_LAYOUT_H
#define GS_LAYOUT_H
#include <stddef.h>

namespace gs_layout {

enum Array { X = 0, Y, A, B, GAMMA, R, S, T, TARGET, XCOMS, YCOMS, PI, THETA, OK, NARRAYS };
static const char* const kArrayName[NARRAYS] = {"X",      "Y",     "A",     "B",  "Gamma", "R",  "S",
                                                "T",      "target", "xcoms", "ycoms", "pi", "theta", "ok"};
static const size_t FR = 32;  // an Fr scalar, on both curves

// equation types as in gs_amd.h: GS_PPE 0, GS_MSMEG1 1, GS_MSMEG2 2, GS_QUAD 3
inline bool x_is_group(int ty) { return ty == 0 || ty == 1; }  // X, A in G1 (else Fr)
inline bool y_is_group(int ty) { return ty == 0 || ty == 2; }  // Y, B in G2 (else Fr)

// the largest shape the engine's task tables take (m, n >= 1 is the caller's to check first)
inline bool shape_fits(int m, int n) { return m <= 4096 && n <= 4096 && (size_t)m * (size_t)n <= ((size_t)1 << 22); }

struct Layout {
  bool xg, yg;
  int kx, ky;         // columns of R = #pi, columns of S = #theta
  size_t sx, sy, st;  // bytes of one X / A element, one Y / B element, one target
  size_t bytes[NARRAYS];
  Layout(size_t fq, int ty, size_t N, int m, int n, bool shared) {
    xg = x_is_group(ty);
    yg = y_is_group(ty);
    kx = xg ? 2 : 1;
    ky = yg ? 2 : 1;
    sx = xg ? 2 * fq : FR;
    sy = yg ? 4 * fq : FR;
    st = ty == 0 ? 12 * fq : ty == 1 ? 2 * fq : ty == 2 ? 4 * fq : FR;
    const size_t V = shared ? 1 : N, um = (size_t)m, un = (size_t)n, ux = (size_t)kx, uy = (size_t)ky;
    bytes[X] = V * um * sx;
    bytes[Y] = V * un * sy;
    bytes[A] = N * un * sx;
    bytes[B] = N * um * sy;
    bytes[GAMMA] = N * um * un * FR;
    bytes[R] = V * um * ux * FR;
    bytes[S] = V * un * uy * FR;
    bytes[T] = N * uy * ux * FR;
    bytes[TARGET] = N * st;
    bytes[XCOMS] = V * um * 4 * fq;  // Com1 = 2 G1
    bytes[YCOMS] = V * un * 8 * fq;  // Com2 = 2 G2
    bytes[PI] = N * ux * 8 * fq;
    bytes[THETA] = N * uy * 4 * fq;
    bytes[OK] = N;
  }
  // bytes of ONE equation's share of every array: what a block of equations [lo, hi) starts at, times lo
  static Layout stride(size_t fq, int ty, int m, int n) { return Layout(fq, ty, 1, m, n, false); }
  // N proofs of ONE equation (gs_verify_equation_rlc): commitments and proofs per proof, the constants A, B, Gamma and
  // the target in one copy
  static Layout one_equation(size_t fq, int ty, size_t N, int m, int n) {
    Layout L(fq, ty, N, m, n, false);
    const Layout one = stride(fq, ty, m, n);
    L.bytes[A] = one.bytes[A];
    L.bytes[B] = one.bytes[B];
    L.bytes[GAMMA] = one.bytes[GAMMA];
    L.bytes[TARGET] = one.bytes[TARGET];
    return L;
  }
};

}  // namespace gs_layout
#endif  // GS_LAYOUT_H
