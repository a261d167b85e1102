// What the multigrid translation units share (csrc/prolong.hip, restrict.hip, coarse_op.hip, coarse_op2.hip, mg_setup.hip, mg_solve.hip,
// coarse_eig.hip): the access to one stored complex number, the member of an aggregate, and two host-side launch
// helpers.  The promises these files make together rest on the single definitions here: products and sums in fp64
// whatever the storage, one rounding on the store, a summation order fixed by the shape of the transfer alone.
#pragma once
#include "internal.h"

namespace mugiq {

// ---- one complex number of storage F: widened to fp64 on the load, rounded once from fp64 on the store (F = double: the same bits both
// ways).  One vec2 access per number, in the global address space
template <typename F> __device__ inline Cplx<double> ld_wide(const void *base, int64_t i) {
  typedef F vec2 __attribute__((ext_vector_type(2)));
  const vec2 t = *as_global(reinterpret_cast<const vec2 *>(base) + i);
  return Cplx<double>{(double)t.x, (double)t.y};
}
template <typename F> __device__ inline void st_round(void *base, int64_t i, const Cplx<double> &v) {
  typedef F vec2 __attribute__((ext_vector_type(2)));
  vec2 t;
  t.x = (F)v.re;
  t.y = (F)v.im;
  *as_global(reinterpret_cast<vec2 *>(base) + i) = t;
}
// ... through a typed pointer, which gives F
template <typename F> __device__ inline Cplx<double> ld_wide(const Cplx<F> *p, int64_t i) { return ld_wide<F>(static_cast<const void *>(p), i); }
template <typename F> __device__ inline void st_round(Cplx<F> *p, int64_t i, const Cplx<double> &v) { st_round<F>(static_cast<void *>(p), i, v); }

// ---- member k (lexicographic inside the block, x fastest) of the aggregate of extents bs at coarse coordinates cc, on the finer lattice
// X: its parity and checkerboard index.  (The Galerkin builds of csrc/coarse_op.hip and csrc/coarse_op2.hip and the row table of
// csrc/mg_setup.hip keep their own walks, which also need the coordinates: through this function their kernels compiled to other code.)
__device__ __forceinline__ void aggregate_member(const int bs[4], const int X[4], const int cc[4], int k, int *pty, int *x_cb) {
  int x[4];
#pragma unroll
  for (int d = 0; d < 4; d++) {
    x[d] = cc[d] * bs[d] + k % bs[d];
    k /= bs[d];
  }
  *pty = (x[0] + x[1] + x[2] + x[3]) & 1;
  *x_cb = lex_index(x, X) >> 1;
}

// ---- a launch with the dynamic LDS it asks for: past 64 KB a kernel has to be told
template <typename Kernel, typename Args> int launch_with_lds(Kernel kern, dim3 grid, int threads, size_t ldsBytes, hipStream_t stream, const Args &a) {
  if (ldsBytes > 64 * 1024)
    MUGIQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes));
  hipLaunchKernelGGL(kern, grid, dim3(threads), ldsBytes, stream, a);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

// ---- a storage precision (4 | 8, validated by the caller) as a value of its type, for a generic lambda:
//     with_storage(p, [&](auto f) { using F = decltype(f); ... }),   with_storage(pv, ps, [&](auto fv, auto fs) { ... })
template <typename Fn> auto with_storage(int precision, Fn &&fn) { return precision == 8 ? fn(double()) : fn(float()); }
template <typename Fn> auto with_storage(int p0, int p1, Fn &&fn) {
  return with_storage(p0, [&](auto f0) { return with_storage(p1, [&](auto f1) { return fn(f0, f1); }); });
}

}  // namespace mugiq
