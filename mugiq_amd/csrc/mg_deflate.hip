// The deflated coarsest solve of the MG cycle: the projection of a coarse right-hand side on the lowest singular triplets (sigma_n, u_n,
// w_n) of the coarsest operator M_L,
//     c_n = <u_n, b>,   x0 = sum_n w_n c_n / sigma_n,   r0 = b - sum_n u_n c_n,
// from which the GCR of csrc/mg_solve.hip starts (MgSolver::gcr_fixed), and the construction of U and sigma from W.  Definitions, promises
// and work memory: MugiqHipCoarseDeflation in include/mugiq_hip.h.  No operator is applied: that is why U is stored.
//
// A field is the list of rows of csrc/mg_common.h (MgLayout; W, U and the right-hand sides each with a stride of their own), a lane
// takes one whole complex number per access, widened to fp64 on the load; every product and sum is fp64 and the store rounds once.
//
//   pass 1  mg_defl_overlap_kernel: grid = element chunks x groups of 16 eigenvectors.  A wave owns 4 eigenvectors and walks the chunk
//           64 elements at a time: the <= 8 right-hand sides of the block at those elements (8 loads, shared through L1 by the four waves
//           of the workgroup, which walk the same chunk) and its 4 eigenvectors (4 loads), 32 complex accumulators per lane.  Per lane
//           in ascending element order, then down the wave by shuffles; the wave's lane 0 writes the chunk's partial sums.  No LDS.
//           mg_defl_coef_kernel adds the partials in ascending chunk order, one lane per (n, r), and forms c and c / sigma.  The chunk
//           length is a function of the elements per vector alone, and every (n, r) has accumulators of its own: the bits of c[n][r]
//           depend on u_n, b_r and the geometry, not on nEv, the batch or the mask.  No atomics.
//   pass 2  mg_defl_combine_kernel: one element per lane and all right-hand sides of the block; w_n and u_n stream by in ascending n, four
//           of each in flight, the coefficients come through scalar loads; x0 and r0 are written once.
//
// Byte model.  Pass 1 reads U once per block: nEv E 2 sizeof(F) bytes for E elements per vector, against 8 right-hand sides x 8 flop per
// complex of U -- 4 flop per byte in fp64 storage, below the ridge of the vector pipe (69 Tflop/s fp64 over the 5.5 TB/s a streaming
// read reaches: 13 flop per byte), so the products stay on the vector pipe and the matrix pipe is not used.
// The right-hand sides are read once per group of 16 eigenvectors
// (8 E 2 sizeof(F) bytes, L2-resident at the shapes of a coarse level: 25 MB at E = 196 608).  Pass 2 reads W and U once and b once, and
// writes x0 and r0: (2 nEv + 8 + 16) E 2 sizeof(F) bytes.  At E = 196 608, nEv = 200: 96 chunks x 13 groups = 1248 workgroups in pass 1,
// 768 in pass 2; 0.63 GB + 1.3 GB in fp64.
#include "mg_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace mugiq {
namespace {

constexpr int kDfThreads = 256;
constexpr int kDfWaveEv = 4;                                  // eigenvectors a wave of pass 1 owns
constexpr int kDfGroupEv = kDfWaveEv * (kDfThreads / 64);     // ... and a workgroup
constexpr int kDfMinChunk = 2048, kDfMaxChunks = 256;          // complex elements per chunk at least; chunks per vector at most
constexpr int kDfMaxEv = 1024;

typedef Cplx<double> Z;

// elements per chunk: a function of the elements per vector alone
int64_t chunk_elems(int64_t total) { return std::max<int64_t>(kDfMinChunk, 64 * ((total + 64 * kDfMaxChunks - 1) / (64 * kDfMaxChunks))); }

__device__ inline double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// partial[chunk][n][r] = sum over the chunk's elements of conj(u_n) b_r, for the active r
template <typename F, typename I>
__global__ __launch_bounds__(kDfThreads) void mg_defl_overlap_kernel(const void *const *Up, MgVecs<F> B, int nEv, MgLayout LU, MgLayout LF, int64_t chunkElems,
                                                                    unsigned active, double *partial) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n0 = ((int)blockIdx.y * (kDfThreads / 64) + w) * kDfWaveEv;
  if (n0 >= nEv) return;  // (wave-uniform; the kernel has no barrier)
  const auto *Uc = as_constant(Up);
  const Cplx<F> *u[kDfWaveEv];
#pragma unroll
  for (int j = 0; j < kDfWaveEv; j++) u[j] = static_cast<const Cplx<F> *>(Uc[min(n0 + j, nEv - 1)]);
  Z acc[kDfWaveEv][kMgBlock];
#pragma unroll
  for (int j = 0; j < kDfWaveEv; j++)
#pragma unroll
    for (int r = 0; r < kMgBlock; r++) acc[j][r] = Z{0.0, 0.0};
  const I e0 = (I)blockIdx.x * (I)chunkElems, e1 = (I)min((int64_t)LF.total, (int64_t)e0 + chunkElems);
  for (I e = e0 + (I)lane; e < e1; e += 64) {
    const MgPlace<I> at(LF, e);
    const int64_t offB = at.in(LF), offU = at.in(LU);
    Z b[kMgBlock];
#pragma unroll
    for (int r = 0; r < kMgBlock; r++) b[r] = ((active >> r) & 1u) ? ld_wide(B.p[r], offB) : Z{0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kDfWaveEv; j++) {
      if (n0 + j < nEv) {
        const Z uu = ld_wide(u[j], offU);
#pragma unroll
        for (int r = 0; r < kMgBlock; r++)
          if ((active >> r) & 1u) cmadd_conj(acc[j][r], uu, b[r]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kDfWaveEv; j++) {
    if (n0 + j < nEv) {
#pragma unroll
      for (int r = 0; r < kMgBlock; r++) {
        if ((active >> r) & 1u) {
          const double re = wave_sum(acc[j][r].re), im = wave_sum(acc[j][r].im);
          if (lane == 0) {
            double *out = partial + (((size_t)blockIdx.x * nEv + (n0 + j)) * kMgBlock + r) * 2;
            out[0] = re;
            out[1] = im;
          }
        }
      }
    }
  }
}

// c[n][r] = sum over the chunks in ascending order, cs[n][r] = c[n][r] / sigma_n; zero for an inactive r (its partials were not written)
__global__ __launch_bounds__(kDfThreads) void mg_defl_coef_kernel(const double *partial, int nChunks, int nEv, const double *sigma, unsigned active, double *c,
                                                                 double *cs) {
  const int i = blockIdx.x * kDfThreads + threadIdx.x;
  if (i >= nEv * kMgBlock) return;
  const int n = i / kMgBlock, r = i - n * kMgBlock;
  double re = 0.0, im = 0.0;
  if ((active >> r) & 1u) {
    for (int k = 0; k < nChunks; k++) {
      const double *p = partial + ((size_t)k * nEv * kMgBlock + i) * 2;
      re += p[0];
      im += p[1];
    }
  }
  const double s = sigma[n];
  c[2 * i] = re;
  c[2 * i + 1] = im;
  cs[2 * i] = re / s;
  cs[2 * i + 1] = im / s;
}

// x0_r = sum_n w_n cs[n][r], r0_r = b_r - sum_n u_n c[n][r] at one element per lane, n ascending; R0.p[r] may be B.p[r]
template <typename F, typename I>
__global__ __launch_bounds__(kDfThreads) void mg_defl_combine_kernel(const void *const *Wp, const void *const *Up, MgVecs<F> X0, MgVecs<F> R0, MgVecs<F> B, int nEv,
                                                                    MgLayout LW, MgLayout LU, MgLayout LF, const double *c, const double *cs, unsigned active) {
  const I e = (I)blockIdx.x * kDfThreads + threadIdx.x;
  if (e >= (I)LF.total) return;
  const MgPlace<I> at(LF, e);
  const int64_t offF = at.in(LF), offW = at.in(LW), offU = at.in(LU);
  const auto *Wc = as_constant(Wp);
  const auto *Uc = as_constant(Up);
  const auto *cc = as_constant(c);
  const auto *sc = as_constant(cs);
  Z x[kMgBlock], r[kMgBlock];
#pragma unroll
  for (int v = 0; v < kMgBlock; v++) {
    x[v] = Z{0.0, 0.0};
    r[v] = ((active >> v) & 1u) ? ld_wide(B.p[v], offF) : Z{0.0, 0.0};
  }
  auto add = [&](int n, const Z &wn, const Z &un) {
#pragma unroll
    for (int v = 0; v < kMgBlock; v++) {
      if ((active >> v) & 1u) {
        const int i = 2 * (n * kMgBlock + v);
        cmadd(x[v], Z{sc[i], sc[i + 1]}, wn);
        cmadd(r[v], Z{-cc[i], -cc[i + 1]}, un);
      }
    }
  };
  constexpr int P = 4;  // eigenvectors in flight
  int n = 0;
  for (; n + P <= nEv; n += P) {
    Z wn[P], un[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
      wn[p] = ld_wide(static_cast<const Cplx<F> *>(Wc[n + p]), offW);
      un[p] = ld_wide(static_cast<const Cplx<F> *>(Uc[n + p]), offU);
    }
#pragma unroll
    for (int p = 0; p < P; p++) add(n + p, wn[p], un[p]);
  }
  for (; n < nEv; n++) add(n, ld_wide(static_cast<const Cplx<F> *>(Wc[n]), offW), ld_wide(static_cast<const Cplx<F> *>(Uc[n]), offU));
#pragma unroll
  for (int v = 0; v < kMgBlock; v++) {
    if ((active >> v) & 1u) {
      st_round(X0.p[v], offF, x[v]);
      st_round(R0.p[v], offF, r[v]);
    }
  }
}

// ---- building U: the squared norm of u_v per wave and chunk, their sum in ascending order, the scaling
template <typename F, typename I>
__global__ __launch_bounds__(kDfThreads) void mg_defl_norm_kernel(MgVecs<F> U, MgLayout L, int64_t chunkElems, double *partial) {
  const int v = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const I e0 = (I)blockIdx.x * (I)chunkElems, e1 = (I)min((int64_t)L.total, (int64_t)e0 + chunkElems);
  double acc = 0.0;
  for (I e = e0 + (I)threadIdx.x; e < e1; e += kDfThreads) {
    const Z u = ld_wide(U.p[v], mg_offset<I>(L, e));
    acc = fma(u.re, u.re, acc);
    acc = fma(u.im, u.im, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) partial[((size_t)v * gridDim.x + blockIdx.x) * (kDfThreads / 64) + w] = acc;
}
__global__ void mg_defl_sigma_kernel(const double *partial, int nPartial, int n, double *sigma) {
  const int v = threadIdx.x;
  if (v >= n) return;
  double a = 0.0;
  for (int k = 0; k < nPartial; k++) a += partial[(size_t)v * nPartial + k];
  sigma[v] = sqrt(a);
}
// u_v /= sigma_v where sigma_v is positive and finite (otherwise the call fails, and u_v stays M w_v)
template <typename F, typename I> __global__ __launch_bounds__(kDfThreads) void mg_defl_scale_kernel(MgVecs<F> U, MgLayout L, const double *sigma) {
  const int v = blockIdx.y;
  const double s = sigma[v];
  if (!(s > 0.0) || !(s < INFINITY)) return;
  const I e = (I)blockIdx.x * kDfThreads + threadIdx.x;
  if (e >= (I)L.total) return;
  const int64_t off = mg_offset<I>(L, e);
  const Z u = ld_wide(U.p[v], off);
  st_round(U.p[v], off, Z{u.re / s, u.im / s});
}

template <typename F> MgVecs<F> bodies(const MugiqHipCoarseField *f, int n) {
  MgVecs<F> m{};
  for (int i = 0; i < n; i++) m.p[i] = static_cast<Cplx<F> *>(f[i].data);
  return m;
}
unsigned grid_of(int64_t total) { return (unsigned)((total + kDfThreads - 1) / kDfThreads); }

#define MUGIQ_DF_LAUNCH(kernel, narrow, grid, ...)                                                                     \
  do {                                                                                                                 \
    if (narrow) hipLaunchKernelGGL((kernel<F, uint32_t>), grid, dim3(kDfThreads), 0, stream, __VA_ARGS__);             \
    else hipLaunchKernelGGL((kernel<F, int64_t>), grid, dim3(kDfThreads), 0, stream, __VA_ARGS__);                     \
    MUGIQ_CHECK_HIP(hipGetLastError());                                                                                \
  } while (0)

template <typename F>
int project(const CoarseDeflationWork &w, const MugiqHipCoarseField *x0, const MugiqHipCoarseField *r0, const MugiqHipCoarseField *b, int n, unsigned active,
            hipStream_t stream) {
  const bool narrow = !w.wide && w.LF.total < (int64_t(1) << 31);
  const MgVecs<F> xv = bodies<F>(x0, n), rv = bodies<F>(r0, n), bv = bodies<F>(b, n);
  MUGIQ_DF_LAUNCH(mg_defl_overlap_kernel, narrow, dim3(w.nChunks, (w.nEv + kDfGroupEv - 1) / kDfGroupEv), w.Up, bv, w.nEv, w.LU, w.LF, w.chunkElems, active,
                  w.partial);
  hipLaunchKernelGGL(mg_defl_coef_kernel, dim3((w.nEv * kMgBlock + kDfThreads - 1) / kDfThreads), dim3(kDfThreads), 0, stream, w.partial, w.nChunks, w.nEv,
                     w.sigma, active, w.c, w.cs);
  MUGIQ_CHECK_HIP(hipGetLastError());
  MUGIQ_DF_LAUNCH(mg_defl_combine_kernel, narrow, dim3(grid_of(w.LF.total)), w.Wp, w.Up, xv, rv, bv, w.nEv, w.LW, w.LU, w.LF, w.c, w.cs, active);
  return MUGIQ_HIP_SUCCESS;
}

// U_i = M w_i / ||M w_i|| for one block of n <= 8, sigma to the host; scal: 8 (4 nChunks + 1) doubles
template <typename F>
int build_block(const MugiqHipCoarseField *U, double *sigma_h, const MugiqHipCoarseField *W, int n, const MugiqHipCoarseOperator *op, double *scal, bool wide,
                hipStream_t stream) {
  if (int st = coarse_apply(U, W, n, op, MUGIQ_HIP_EIG_OPERATOR_M, 1.0, stream)) return st;
  const MgLayout L = coarse_layout(U[0]);
  const bool narrow = !wide && L.total < (int64_t(1) << 31);
  const int64_t ce = chunk_elems(L.total);
  const int nChunks = (int)((L.total + ce - 1) / ce), nPartial = nChunks * (kDfThreads / 64);
  double *sigma_d = scal + (size_t)kMgBlock * nPartial;
  const MgVecs<F> uv = bodies<F>(U, n);
  MUGIQ_DF_LAUNCH(mg_defl_norm_kernel, narrow, dim3(nChunks, n), uv, L, ce, scal);
  hipLaunchKernelGGL(mg_defl_sigma_kernel, dim3(1), dim3(64), 0, stream, scal, nPartial, n, sigma_d);
  MUGIQ_CHECK_HIP(hipGetLastError());
  MUGIQ_DF_LAUNCH(mg_defl_scale_kernel, narrow, dim3(grid_of(L.total), n), uv, L, sigma_d);
  MUGIQ_CHECK_HIP(hipMemcpyAsync(sigma_h, sigma_d, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
  MUGIQ_CHECK_HIP(hipStreamSynchronize(stream));
  return MUGIQ_HIP_SUCCESS;
}
#undef MUGIQ_DF_LAUNCH

bool good_sigma(double s) { return s > 0.0 && std::isfinite(s); }

}  // namespace

int check_coarse_deflation(const MugiqHipCoarseDeflation *d, const MugiqHipCoarseOperator *op, const uintptr_t (*fields)[2], int nFields, const char *who) {
  MUGIQ_REQUIRE(d->nEv >= 1 && d->nEv <= kDfMaxEv, "%s: deflation nEv = %d must be in [1, %d]", who, d->nEv, kDfMaxEv);
  MUGIQ_REQUIRE(d->W != nullptr && d->U != nullptr && d->sigma != nullptr, "%s: deflation W, U or sigma is NULL", who);
  int st;
  if ((st = validate_coarse_vectors(d->W, d->nEv, op, who, "deflation W"))) return st;
  if ((st = validate_coarse_vectors(d->U, d->nEv, op, who, "deflation U"))) return st;
  // [first, last) of every body, W then U: none shares a byte with another or with a field of the call
  std::vector<uintptr_t> a(2 * (size_t)d->nEv), b(2 * (size_t)d->nEv);
  for (int n = 0; n < d->nEv; n++) {
    coarse_span(d->W[n], &a[n], &b[n]);
    coarse_span(d->U[n], &a[d->nEv + n], &b[d->nEv + n]);
  }
  auto name = [&](size_t i) { return i < (size_t)d->nEv ? "W" : "U"; };
  for (size_t i = 0; i < a.size(); i++) {
    for (size_t j = 0; j < i; j++)
      MUGIQ_REQUIRE(!(a[i] < b[j] && a[j] < b[i]), "%s: deflation %s vector %d overlaps deflation %s vector %d", who, name(i), (int)(i % d->nEv), name(j),
                    (int)(j % d->nEv));
    for (int f = 0; f < nFields; f++)
      MUGIQ_REQUIRE(!(a[i] < fields[f][1] && fields[f][0] < b[i]), "%s: deflation %s vector %d overlaps field %d of the call", who, name(i), (int)(i % d->nEv), f);
  }
  for (int n = 0; n < d->nEv; n++) MUGIQ_REQUIRE(good_sigma(d->sigma[n]), "%s: deflation sigma[%d] = %g must be positive and finite", who, n, d->sigma[n]);
  return MUGIQ_HIP_SUCCESS;
}

size_t coarse_deflation_work_bytes(const MugiqHipCoarseField &like, int nEv) {
  const int64_t total = coarse_layout(like).total, ce = chunk_elems(total);
  const size_t nChunks = (size_t)((total + ce - 1) / ce);
  return align256(sizeof(double) * (size_t)nEv * (3 + 4 * kMgBlock + 2 * kMgBlock * nChunks));
}

int coarse_deflation_prepare(CoarseDeflationWork *w, const MugiqHipCoarseDeflation *d, const MugiqHipCoarseField &like, void *mem, bool wide, hipStream_t stream) {
  static_assert(sizeof(void *) == sizeof(double), "the body tables are laid out in words of 8 bytes");
  const int nEv = d->nEv;
  w->nEv = nEv, w->wide = wide;
  w->LW = coarse_layout(d->W[0]), w->LU = coarse_layout(d->U[0]), w->LF = coarse_layout(like);
  w->chunkElems = chunk_elems(w->LF.total);
  w->nChunks = (int)((w->LF.total + w->chunkElems - 1) / w->chunkElems);
  // sigma | bodies of W | bodies of U | c | c / sigma | partials; the first three go up once, through the stream's table buffer
  double *base = static_cast<double *>(mem);
  w->sigma = base;
  w->Wp = reinterpret_cast<const void *const *>(base + nEv);
  w->Up = reinterpret_cast<const void *const *>(base + 2 * (size_t)nEv);
  w->c = base + 3 * (size_t)nEv;
  w->cs = w->c + 2 * (size_t)kMgBlock * nEv;
  w->partial = w->cs + 2 * (size_t)kMgBlock * nEv;
  std::vector<double> host(3 * (size_t)nEv);
  const void **tab = reinterpret_cast<const void **>(host.data() + nEv);
  for (int n = 0; n < nEv; n++) {
    host[n] = d->sigma[n];
    tab[n] = d->W[n].data;
    tab[nEv + n] = d->U[n].data;
  }
  void *staged = nullptr;
  if (int st = upload_table(&staged, host.data(), sizeof(double) * host.size(), stream)) return st;
  MUGIQ_CHECK_HIP(hipMemcpyAsync(mem, staged, sizeof(double) * host.size(), hipMemcpyDeviceToDevice, stream));
  return MUGIQ_HIP_SUCCESS;
}

int coarse_deflation_project(const CoarseDeflationWork &w, const MugiqHipCoarseField *x0, const MugiqHipCoarseField *r0, const MugiqHipCoarseField *b, int n,
                             unsigned active, int precision, hipStream_t stream) {
  return with_storage(precision, [&](auto f) { return project<decltype(f)>(w, x0, r0, b, n, active, stream); });
}

}  // namespace mugiq

using namespace mugiq;

extern "C" {

int mugiq_hip_coarse_deflation_build(const MugiqHipCoarseField *U_h, double *sigma_h, const MugiqHipCoarseField *W_h, int nEv, const MugiqHipCoarseOperator *op,
                                     const MugiqHipComm *comm, void *stream) {
  const char *who = "coarseDeflationBuild";
  MUGIQ_REQUIRE(U_h != nullptr && sigma_h != nullptr && W_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nEv >= 1 && nEv <= kDfMaxEv, "%s: nEv = %d must be in [1, %d]", who, nEv, kDfMaxEv);
  int st;
  if ((st = check_single_domain(comm, who))) return st;
  if ((st = validate_coarse_operator(op, who))) return st;
  if ((st = validate_coarse_vectors(W_h, nEv, op, who, "W"))) return st;
  if ((st = validate_coarse_vectors(U_h, nEv, op, who, "U"))) return st;
  for (int i = 0; i < nEv; i++) {
    uintptr_t a0, a1, b0, b1;
    coarse_span(U_h[i], &a0, &a1);
    for (int j = 0; j < nEv; j++) {
      coarse_span(W_h[j], &b0, &b1);
      MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1), "%s: U vector %d overlaps W vector %d", who, i, j);
      if (j < i) {
        coarse_span(U_h[j], &b0, &b1);
        MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1), "%s: U vector %d overlaps U vector %d", who, i, j);
      }
    }
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  void *scal = nullptr;
  if ((st = stream_operator_workspace(&scal, sizeof(double) * kMgBlock * ((size_t)kDfMaxChunks * (kDfThreads / 64) + 1), s))) return st;
  const bool wide = debug_wide_index_asked();
  for (int n0 = 0; n0 < nEv; n0 += kMgBlock) {
    const int n = std::min(kMgBlock, nEv - n0);
    st = with_storage(op->precision, [&](auto f) { return build_block<decltype(f)>(U_h + n0, sigma_h + n0, W_h + n0, n, op, static_cast<double *>(scal), wide, s); });
    if (st) return st;
  }
  for (int n = 0; n < nEv; n++) MUGIQ_REQUIRE(good_sigma(sigma_h[n]), "%s: sigma[%d] = ||M w|| = %g is not positive and finite (sigma_h is filled)", who, n, sigma_h[n]);
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_coarse_deflate(const MugiqHipCoarseField *x0_h, const MugiqHipCoarseField *r0_h, const MugiqHipCoarseField *b_h, int nVec,
                             const MugiqHipCoarseDeflation *space, const MugiqHipComm *comm, void *stream) {
  const char *who = "coarseDeflate";
  MUGIQ_REQUIRE(x0_h != nullptr && r0_h != nullptr && b_h != nullptr && space != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nVec >= 1, "%s: nVec = %d must be >= 1", who, nVec);
  int st;
  if ((st = check_single_domain(comm, who))) return st;
  MUGIQ_REQUIRE(space->nEv >= 1 && space->nEv <= kDfMaxEv, "%s: deflation nEv = %d must be in [1, %d]", who, space->nEv, kDfMaxEv);
  MUGIQ_REQUIRE(space->W != nullptr && space->U != nullptr && space->sigma != nullptr, "%s: deflation W, U or sigma is NULL", who);
  MUGIQ_REQUIRE(space->W[0].data != nullptr, "%s: deflation W vector 0 is NULL", who);
  // the space's own lattice, n_vec and precision stand for the operator: W[0] describes them, and everything else is held to it
  const MugiqHipCoarseField &w0 = space->W[0];
  MugiqHipCoarseOperator geo{};
  geo.data = w0.data, geo.precision = w0.precision, geo.nVec = w0.nColor, geo.volumeCB = w0.volumeCB;
  for (int d = 0; d < 4; d++) geo.X[d] = w0.X[d];
  if ((st = validate_coarse_operator(&geo, who))) return st;
  const MugiqHipCoarseField *sets[3] = {x0_h, r0_h, b_h};
  const char *names[3] = {"x0", "r0", "b"};
  std::vector<uintptr_t> span(2 * 3 * (size_t)nVec);
  uintptr_t(*fields)[2] = reinterpret_cast<uintptr_t(*)[2]>(span.data());
  for (int k = 0; k < 3; k++) {
    if ((st = validate_coarse_vectors(sets[k], nVec, &geo, who, names[k]))) return st;
    MUGIQ_REQUIRE(sets[k][0].stride == x0_h[0].stride && sets[k][0].parity_offset == x0_h[0].parity_offset,
                  "%s: x0, r0 and b must have one stride and parity offset", who);
    for (int i = 0; i < nVec; i++) coarse_span(sets[k][i], &fields[k * nVec + i][0], &fields[k * nVec + i][1]);
  }
  for (int i = 0; i < 3 * nVec; i++)
    for (int j = 0; j < i; j++)
      MUGIQ_REQUIRE(!(fields[i][0] < fields[j][1] && fields[j][0] < fields[i][1]), "%s: %s vector %d overlaps %s vector %d", who, names[i / nVec], i % nVec,
                    names[j / nVec], j % nVec);
  if ((st = check_coarse_deflation(space, &geo, fields, 3 * nVec, who))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  void *mem = nullptr;
  if ((st = stream_operator_workspace(&mem, coarse_deflation_work_bytes(b_h[0], space->nEv), s))) return st;
  CoarseDeflationWork w;
  if ((st = coarse_deflation_prepare(&w, space, b_h[0], mem, debug_wide_index_asked(), s))) return st;
  for (int v0 = 0; v0 < nVec; v0 += kMgBlock) {
    const int n = std::min(kMgBlock, nVec - v0);
    if ((st = coarse_deflation_project(w, x0_h + v0, r0_h + v0, b_h + v0, n, (1u << n) - 1u, w0.precision, s))) return st;
  }
  return MUGIQ_HIP_SUCCESS;
}

}  // extern "C"
