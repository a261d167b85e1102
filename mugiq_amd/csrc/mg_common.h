// What the multigrid translation units share (csrc/prolong.hip, restrict.hip, coarse_op.hip, coarse_op2.hip, mg_setup.hip, mg_solve.hip,
// coarse_eig.hip, mg_deflate.hip): the access to one stored complex number, the member of an aggregate, the walk over a field's
// elements, the deflated coarsest solve's internal entries, and two host-side launch helpers.  The promises these files make together
// rest on the single definitions here: products and sums in fp64 whatever the storage, one rounding on the store, a summation order
// fixed by the shape of the transfer alone.
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

// ---- a field as the Krylov kernels of csrc/mg_solve.hip and the projection of csrc/mg_deflate.hip walk it: rows of complex numbers,
// element e = (parity, row, position in the row) in ascending order, whatever the stride and the parity offset
constexpr int kMgBlock = 8;  // right-hand sides per block
struct MgLayout {
  int nRows;
  int64_t rowLen, rowStride, po, total;  // complex elements; total = 2 nRows rowLen
};

// (parity, row, position in the row) of element e, rows in ascending order: the same in every layout of one geometry (nRows, rowLen),
// whatever its stride and parity offset.  I: uint32_t where total < 2^31
template <typename I> struct MgPlace {
  int pty;
  I row, pos;
  __device__ inline MgPlace(const MgLayout &L, I e) {
    const I rowLen = (I)L.rowLen, per = (I)L.nRows * rowLen;
    pty = e >= per ? 1 : 0;
    const I rem = e - (pty ? per : (I)0);
    row = rem / rowLen;
    pos = rem - row * rowLen;
  }
  // the complex offset of the place in a field laid out as L
  __device__ inline int64_t in(const MgLayout &L) const { return pty * L.po + (int64_t)row * L.rowStride + (int64_t)pos; }
};
// complex offset of element e of a field
template <typename I> __device__ inline int64_t mg_offset(const MgLayout &L, I e) { return MgPlace<I>(L, e).in(L); }

// the bodies of the right-hand sides of a block
template <typename F> struct MgVecs {
  Cplx<F> *p[kMgBlock];
};

inline MgLayout coarse_layout(const MugiqHipCoarseField &f) {
  MgLayout L;
  L.nRows = f.nSpin * f.nColor;
  L.rowLen = f.volumeCB;
  L.rowStride = f.stride;
  L.po = f.parity_offset;
  L.total = 2 * L.nRows * L.rowLen;
  return L;
}

// ---- the deflated coarsest solve (csrc/mg_deflate.hip; definitions: MugiqHipCoarseDeflation in include/mugiq_hip.h) below its C entries,
// for the solver of csrc/mg_solve.hip.  check_coarse_deflation: everything about a space that can be refused, against the operator of its
// level, before any device work; `fields` are byte ranges [a, b) of the call's own fields, which no w_n or u_n may share a byte with.
// CoarseDeflationWork: the space of one call on the device -- sigma, the bodies of W and U, the coefficients [nEv][8] (c and c / sigma)
// and the chunk partials -- in coarse_deflation_work_bytes of the caller's memory, filled once per call by coarse_deflation_prepare.
// coarse_deflation_project: x0_i = sum_n w_n c_ni / sigma_n, r0_i = b_i - sum_n u_n c_ni, c_ni = <u_n, b_i>, for the active i < n <= 8;
// x0, r0 and b have the layout `like` of prepare, r0_i may be b_i itself; two launches and a small one, nothing read back
struct CoarseDeflationWork {
  int nEv = 0, nChunks = 0;
  int64_t chunkElems = 0;
  bool wide = false;
  MgLayout LW, LU, LF;
  const void *const *Wp = nullptr, *const *Up = nullptr;
  const double *sigma = nullptr;
  double *c = nullptr, *cs = nullptr, *partial = nullptr;
};
int check_coarse_deflation(const MugiqHipCoarseDeflation *d, const MugiqHipCoarseOperator *op, const uintptr_t (*fields)[2], int nFields, const char *who);
size_t coarse_deflation_work_bytes(const MugiqHipCoarseField &like, int nEv);
int coarse_deflation_prepare(CoarseDeflationWork *w, const MugiqHipCoarseDeflation *d, const MugiqHipCoarseField &like, void *mem, bool wide, hipStream_t stream);
int coarse_deflation_project(const CoarseDeflationWork &w, const MugiqHipCoarseField *x0, const MugiqHipCoarseField *r0, const MugiqHipCoarseField *b, int n,
                             unsigned active, int precision, hipStream_t stream);

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
