// Device probe of the lazy radix-2^28 arithmetic: a test-only translation unit over the PRODUCT'S headers (it links nothing
// from the library).  One kernel per operation and curve reads raw operand limb vectors, applies the operation lane by
// lane and writes the raw result limbs; tests/test_gpu_arith.py compares them with big integers.  Built by that test with
// the engine's own compile flags (make -s -C groth_sahai_rs_amd/csrc print-flags) plus -I of the header directory, a
// second time with -DGS_NO_ASM_CALL -DARITH_BASE_FP2_ONLY (the inline multiplier forms of the fallback build under the
// base-field and Fp2 families; an operation that is not compiled in returns -2).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gs_params_bls12_381.h"
#include "gs_params_bn254.h"
#include "gs_pairing.cuh"

namespace gs {
GS_ZERO_ONE(Bls12_381)
GS_ZERO_ONE(Bn254)
}
#include "arith_ops.inc"

template <class C, int OP> __global__ void __launch_bounds__(64) k_arith(int n, const int32_t* in, int32_t* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  arith::arith_op<C, OP>(in + (size_t)i * arith::op_nin(OP) * C::L, out + (size_t)i * arith::op_nout(OP) * C::L);
}

template <class C> static int run(int op, int n, const int32_t* in, int32_t* out) {
  if (op < 0 || op >= arith::NUM_OPS || n <= 0) return -1;
  const size_t bin = (size_t)n * arith::op_nin(op) * C::L * sizeof(int32_t);
  const size_t bout = (size_t)n * arith::op_nout(op) * C::L * sizeof(int32_t);
  int32_t *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, bin);
  if (e == hipSuccess) e = hipMalloc(&dout, bout);
  if (e == hipSuccess) e = hipMemcpy(din, in, bin, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xEE, bout);
  if (e == hipSuccess) {
    const dim3 grid((n + 63) / 64), block(64);
    switch (op) {
#define ARITH_CASE(K) \
  case K: hipLaunchKernelGGL((k_arith<C, K>), grid, block, 0, 0, n, din, dout); break;
      ARITH_FOR_EACH_OP(ARITH_CASE)
#undef ARITH_CASE
      default: (void)hipFree(din); (void)hipFree(dout); return -2;
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();  // one launch, no retry: a failure is reported as it is
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, bout, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}

// curve: 0 = BLS12-381, 1 = BN254.  Returns 0, -1 for bad arguments, -2 for an operation left out of this build, or the
// HIP error code.
extern "C" int probe_run(int curve, int op, int n, const int32_t* in, int32_t* out) {
  return curve == 0 ? run<gs::Bls12_381>(op, n, in, out) : run<gs::Bn254>(op, n, in, out);
}
extern "C" int probe_shape(int op, int* nin, int* nout) {
  if (op < 0 || op >= arith::NUM_OPS) return -1;
  *nin = arith::op_nin(op);
  *nout = arith::op_nout(op);
  return 0;
}
