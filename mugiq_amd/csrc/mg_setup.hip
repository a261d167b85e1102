// MG setup on the device: the block orthonormalisation of a transfer's null vectors V (QUDA's BlockOrthogonalize), the kernels that pack
// fine vectors into V and read them back, the orthonormality check, and the host driver that makes V from a gauge field with the
// library's own operator, CG and two-grid solve.  Contracts: mugiq_hip_block_orthonormalize and mugiq_hip_mg_setup in include/mugiq_hip.h.
//
// block_ortho_kernel: one workgroup of 256 lanes per block B (an aggregate and a coarse spin), m rows x n_vec columns.  The kernel sees a
// block as a list of rows: row r = k aggVol + a is the spin-colour row k < K of the block's site a, sites in the lexicographic order of
// their LOCAL coordinates in the aggregate (x fastest).  The offset of every row comes from a table in LDS (8 m bytes), filled once from
// the level geometry; K = 6 on the finest level (rows 3 s + c of one chirality), K = nColor of the finer side on a coarse -> coarse level.
// A left-looking walk: column j is widened to fp64 into LDS (16 m bytes; lane t keeps rows t, t + 256, ...), the finished columns q_i are
// re-read from global memory, 16 of them per reduction round (the block is 590 KB at m = 1536 and n_vec = 24 in fp64; with four workgroups
// on every CU the blocks in flight exceed the caches at 32^4, so these re-reads are what the kernel's time goes into: DESIGN.md 4.4d).
// Every sum runs per lane over its rows in ascending order, down the wave by shuffles and over the four waves in ascending order: the order depends on m alone, so a block has the same bits in every lattice and beside any other blocks.
#include "mg_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace mugiq {
namespace {

constexpr int kBoThreads = 256;
constexpr int kBoWaves = kBoThreads / 64;
constexpr int kBoChunk = 16;                  // finished columns per reduction round
constexpr int kBoSlots = 2 * kBoChunk + 1;    // their complex coefficients and one norm
constexpr int kBoMaxNV = 96;                  // n_vec of a coarse -> coarse level (validate_coarse_transfer)
constexpr int kSetupBlock = 8;                // vectors per call of the batched operator and solvers
constexpr int kSetupMaxNV = 64;               // n_vec of a finest-level transfer: MugiqHipMgSetupInfo::cgIters

typedef Cplx<double> Z;

struct BoArgs {
  void *V;
  int64_t po;
  int stride, nVec;
  int X[4], Xc[4], bs[4];
  int aggVol, K, m, nPasses;
  double *blockRatio;  // [blocks] the smallest first-pass nu_j / ||b_j as given||
  int *blockZeros;     // [blocks] columns stored as zeros
  double *blockDev;    // [blocks] max |B^dag B - 1| (ortho_check_kernel)
};

// v[0 .. nUsed) summed over the workgroup -> out[0 .. nUsed) in LDS, visible to every lane on return
__device__ inline void bo_group_sum(double (&v)[kBoSlots], int nUsed, double (*red)[kBoSlots], double *out) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int s = 0; s < kBoSlots; s++) {
    if (s < nUsed) {
      double x = v[s];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
      if (lane == 0) red[w][s] = x;
    }
  }
  __syncthreads();
  if (t < nUsed) out[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  __syncthreads();
}

// the row table of block `blk` = 2 aggregate + S: rowBase[r] = the offset of column 0 of row r = k aggVol + a, i.e.
// parity po + x_cb of site a plus the rows (K S + k) n_vec in front of it
__device__ inline void bo_row_table(const BoArgs &A, int blk, int64_t *rowBase) {
  const int S = blk & 1;
  int agg = blk >> 1, cX[4];
#pragma unroll
  for (int d = 0; d < 4; d++) {
    cX[d] = agg % A.Xc[d];
    agg /= A.Xc[d];
  }
  for (int r = threadIdx.x; r < A.m; r += kBoThreads) {
    const int k = r / A.aggVol;
    int rem = r - k * A.aggVol, c[4], sum = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const int l = rem % A.bs[d];
      rem /= A.bs[d];
      c[d] = cX[d] * A.bs[d] + l;
      sum += c[d];
    }
    rowBase[r] = (int64_t)(sum & 1) * A.po + (lex_index(c, A.X) >> 1) + (int64_t)(A.K * S + k) * A.nVec * A.stride;
  }
  __syncthreads();
}

// the smaller of a and b, and NaN if either is one
__device__ inline double bo_min_keep_nan(double a, double b) { return (b < a || b != b) ? b : a; }

// <q_i, col> for i0 <= i < i0 + nc into acc[2 (i - i0)], acc[2 (i - i0) + 1]
template <typename F> __device__ inline void bo_dots(const BoArgs &A, const int64_t *rowBase, const Z *col, int i0, int nc, double (&acc)[kBoSlots]) {
  for (int r = threadIdx.x; r < A.m; r += kBoThreads) {
    const Z b = col[r];
    const int64_t base = rowBase[r] + (int64_t)i0 * A.stride;
#pragma unroll
    for (int ii = 0; ii < kBoChunk; ii++) {
      if (ii < nc) {
        const Z q = ld_wide<F>(A.V, base + (int64_t)ii * A.stride);
        acc[2 * ii] = fma(q.re, b.re, acc[2 * ii]);
        acc[2 * ii] = fma(q.im, b.im, acc[2 * ii]);
        acc[2 * ii + 1] = fma(q.re, b.im, acc[2 * ii + 1]);
        acc[2 * ii + 1] = fma(-q.im, b.re, acc[2 * ii + 1]);
      }
    }
  }
}

template <typename F> __global__ __launch_bounds__(kBoThreads) void block_ortho_kernel(BoArgs A) {
  extern __shared__ __align__(16) unsigned char bo_lds[];
  Z *col = reinterpret_cast<Z *>(bo_lds);
  int64_t *rowBase = reinterpret_cast<int64_t *>(col + A.m);
  __shared__ double red[kBoWaves][kBoSlots], sums[kBoSlots];
  __shared__ Z coef[kBoMaxNV];
  const int t = threadIdx.x, blk = blockIdx.x;
  bo_row_table(A, blk, rowBase);
  double minRatio = INFINITY;
  int zeros = 0;
  for (int pass = 0; pass < A.nPasses; pass++) {
    for (int j = 0; j < A.nVec; j++) {
      // b_j as given, and its norm
      double acc[kBoSlots];
#pragma unroll
      for (int s = 0; s < kBoSlots; s++) acc[s] = 0.0;
      for (int r = t; r < A.m; r += kBoThreads) {
        const Z b = ld_wide<F>(A.V, rowBase[r] + (int64_t)j * A.stride);
        col[r] = b;
        acc[2 * kBoChunk] = fma(b.re, b.re, acc[2 * kBoChunk]);
        acc[2 * kBoChunk] = fma(b.im, b.im, acc[2 * kBoChunk]);
      }
      // c_i = <q_i, b_j> for all i < j from the un-updated b_j, 16 to a round; the first round carries ||b_j||^2
      double given2 = 0.0;
      int i0 = 0;
      do {
        const int nc = min(kBoChunk, j - i0);
        bo_dots<F>(A, rowBase, col, i0, nc, acc);
        bo_group_sum(acc, i0 == 0 ? kBoSlots : 2 * nc, red, sums);
        if (i0 == 0) given2 = sums[2 * kBoChunk];
        if (t < nc) coef[i0 + t] = Z{sums[2 * t], sums[2 * t + 1]};
#pragma unroll
        for (int s = 0; s < kBoSlots; s++) acc[s] = 0.0;
        i0 += kBoChunk;
      } while (i0 < j);
      __syncthreads();
      // b_j -= sum_i c_i q_i, nu = ||b_j||
      for (int r = t; r < A.m; r += kBoThreads) {
        Z b = col[r];
        const int64_t base = rowBase[r];
        for (int i = 0; i < j; i++) {
          const Z c = coef[i], mc{-c.re, -c.im};
          cmadd(b, mc, ld_wide<F>(A.V, base + (int64_t)i * A.stride));
        }
        col[r] = b;
        acc[0] = fma(b.re, b.re, acc[0]);
        acc[0] = fma(b.im, b.im, acc[0]);
      }
      bo_group_sum(acc, 1, red, sums);
      const double nu = sqrt(sums[0]);
      if (pass == 0) minRatio = bo_min_keep_nan(minRatio, given2 == 0.0 ? 0.0 : nu / sqrt(given2));
      if (nu == 0.0 && pass == A.nPasses - 1) zeros++;
      // q_j = b_j / nu (nu = 0: exact zeros; a NaN in the column stays one), one rounding on the store
      for (int r = t; r < A.m; r += kBoThreads) {
        const Z b = col[r];
        st_round<F>(A.V, rowBase[r] + (int64_t)j * A.stride, nu != 0.0 ? Z{b.re / nu, b.im / nu} : Z{0.0, 0.0});
      }
      __threadfence_block();
      __syncthreads();  // q_j is in memory before a lane of another wave reads it as a finished column
    }
  }
  if (t == 0) {
    A.blockRatio[blk] = minRatio;
    A.blockZeros[blk] = zeros;
  }
}

// max over the entries of |B^dag B - 1| of every block, by the sums of the kernel above
template <typename F> __global__ __launch_bounds__(kBoThreads) void ortho_check_kernel(BoArgs A) {
  extern __shared__ __align__(16) unsigned char bo_lds[];
  Z *col = reinterpret_cast<Z *>(bo_lds);
  int64_t *rowBase = reinterpret_cast<int64_t *>(col + A.m);
  __shared__ double red[kBoWaves][kBoSlots], sums[kBoSlots], worst[kBoChunk];
  const int t = threadIdx.x, blk = blockIdx.x;
  bo_row_table(A, blk, rowBase);
  double dev = 0.0;
  for (int j = 0; j < A.nVec; j++) {
    for (int r = t; r < A.m; r += kBoThreads) col[r] = ld_wide<F>(A.V, rowBase[r] + (int64_t)j * A.stride);
    for (int i0 = 0; i0 <= j; i0 += kBoChunk) {
      const int nc = min(kBoChunk, j + 1 - i0);
      double acc[kBoSlots];
#pragma unroll
      for (int s = 0; s < kBoSlots; s++) acc[s] = 0.0;
      bo_dots<F>(A, rowBase, col, i0, nc, acc);
      bo_group_sum(acc, 2 * nc, red, sums);
      if (t < nc) {
        const double re = sums[2 * t] - (i0 + t == j ? 1.0 : 0.0), im = sums[2 * t + 1];
        const double d = sqrt(re * re + im * im);
        if (d > dev || d != d) dev = d;
      }
      __syncthreads();
    }
  }
  if (t < kBoChunk) worst[t] = dev;
  __syncthreads();
  if (t == 0) {
    double d = 0.0;
    for (int i = 0; i < kBoChunk; i++)
      if (worst[i] > d || worst[i] != worst[i]) d = worst[i];
    A.blockDev[blk] = d;
  }
}

// what the host reads: the minimum of the ratios, the sum of the zero columns and the maximum of the deviations over the blocks
struct BoResult {
  double minRatio, maxDev;
  long long zeros;
};
__global__ __launch_bounds__(kBoThreads) void block_info_kernel(const double *ratio, const int *zeros, const double *dev, int nBlocks, BoResult *out) {
  __shared__ double shR[kBoThreads], shD[kBoThreads];
  __shared__ long long shZ[kBoThreads];
  const int t = threadIdx.x;
  double r = INFINITY, d = 0.0;
  long long z = 0;
  for (int b = t; b < nBlocks; b += kBoThreads) {
    if (ratio) r = bo_min_keep_nan(r, ratio[b]);
    if (zeros) z += zeros[b];
    if (dev && (dev[b] > d || dev[b] != dev[b])) d = dev[b];
  }
  shR[t] = r, shD[t] = d, shZ[t] = z;
  __syncthreads();
  if (t == 0) {
    for (int i = 1; i < kBoThreads; i++) {
      r = bo_min_keep_nan(r, shR[i]);
      z += shZ[i];
      if (shD[i] > d || shD[i] != shD[i]) d = shD[i];
    }
    out->minRatio = r, out->maxDev = d, out->zeros = z;
  }
}

// ---- V <-> fine vectors.  One lane per (parity, spin-colour k, x_cb), all n_vec columns
struct PackArgs {
  void *V;
  int64_t po;
  int stride, nVec, volumeCB;
  const void *const *vecs;  // device table of the vectors' bodies (pack), or NULL
  void *vec;                // the one vector (unpack)
  int j;
  int vStride;
  int64_t vPo;
};
template <int ORDER> __device__ inline int64_t spinor_elem(int parity, int k, int x, int stride, int64_t po) {
  if constexpr (ORDER == 2) return parity * po + (int64_t)k * stride + x;
  return parity * po + ((int64_t)(k >> 1) * stride + x) * 2 + (k & 1);
}
template <typename FV, typename FS, int ORDER> __global__ __launch_bounds__(256) void pack_vectors_kernel(PackArgs A) {
  const int x = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, parity = blockIdx.z;
  if (x >= A.volumeCB) return;
  const int64_t src = spinor_elem<ORDER>(parity, k, x, A.vStride, A.vPo);
  const int64_t dst = parity * A.po + (int64_t)k * A.nVec * A.stride + x;
  for (int j = 0; j < A.nVec; j++) st_round<FV>(A.V, dst + (int64_t)j * A.stride, ld_wide<FS>(as_constant(A.vecs)[j], src));
}
template <typename FV, typename FS, int ORDER> __global__ __launch_bounds__(256) void unpack_vector_kernel(PackArgs A) {
  const int x = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, parity = blockIdx.z;
  if (x >= A.volumeCB) return;
  st_round<FS>(A.vec, spinor_elem<ORDER>(parity, k, x, A.vStride, A.vPo), ld_wide<FV>(A.V, parity * A.po + ((int64_t)k * A.nVec + A.j) * A.stride + x));
}

// dst = a - b on the bodies of fp64 fields of one layout (rows of rowLen complex numbers rowStride apart; pads are not touched)
struct SubArgs {
  Z *dst;
  const Z *a, *b;
  int nRows;
  int64_t rowLen, rowStride, po;
};
__global__ __launch_bounds__(256) void field_sub_kernel(SubArgs A) {
  const int64_t per = (int64_t)A.nRows * A.rowLen, total = 2 * per;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int pty = e >= per ? 1 : 0;
    const int64_t rem = e - pty * per, row = rem / A.rowLen;
    const int64_t off = pty * A.po + row * A.rowStride + (rem - row * A.rowLen);
    const Z x = ld_wide<double>(A.a, off), y = ld_wide<double>(A.b, off);
    st_round<double>(A.dst, off, Z{x.re - y.re, x.im - y.im});
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
struct BoLevel {
  TransferGeom g;
  int K = 0, m = 0, nBlocks = 0;
  size_t ldsBytes = 0;
};

// the checks of mugiq_hip_prolongate_batched (finest level) or mugiq_hip_prolongate_coarse_batched (coarse -> coarse) on the transfer
// alone, and the block geometry.  A coarse -> coarse V carries the colours of its finer side only in its parity offset, which therefore
// has to be exact: parity_offset = 2 nColor n_vec stride
int bo_level(const MugiqHipTransfer *T, const char *who, BoLevel *out) {
  MUGIQ_REQUIRE(T != nullptr && T->V != nullptr, "%s: transfer / null vectors are NULL", who);
  MUGIQ_REQUIRE(T->spinBlockSize == 1 || T->spinBlockSize == 2, "%s: spin_block_size = %d (2: finest level, 1: coarse -> coarse)", who, T->spinBlockSize);
  for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(T->X[d] > 0 && T->geoBlockSize[d] >= 1, "%s: transfer X / geo_block_size[%d]", who, d);
  BoLevel L;
  L.g = transfer_geom(*T);
  if (T->spinBlockSize == 2) {
    MugiqHipCoarseField c0 = coarse_side_layout(*T);
    c0.data = reinterpret_cast<void *>(uintptr_t(16));  // geometry only: never read
    if (int st = validate_transfer(T, &c0, who)) return st;
    L.K = 6;
  } else {
    MUGIQ_REQUIRE(T->precision == 4 || T->precision == 8, "%s: transfer precision %d", who, T->precision);
    MUGIQ_REQUIRE(T->nVec >= 1 && T->nVec <= kBoMaxNV, "%s: n_vec = %d must be in [1, %d]", who, T->nVec, kBoMaxNV);
    long long vol = 1;
    for (int d = 0; d < 4; d++) {
      MUGIQ_REQUIRE((T->X[d] & 1) == 0, "%s: finer lattice X[%d] = %d must be even", who, d, T->X[d]);
      MUGIQ_REQUIRE(T->X[d] % T->geoBlockSize[d] == 0, "%s: geo_block_size[%d] = %d does not divide X = %d", who, d, T->geoBlockSize[d], T->X[d]);
      MUGIQ_REQUIRE(((T->X[d] / T->geoBlockSize[d]) & 1) == 0, "%s: coarser extent in dim %d must be even", who, d);
      vol *= T->X[d];
    }
    MUGIQ_REQUIRE(T->stride >= vol / 2, "%s: V stride too small", who);
    const int64_t unit = (int64_t)2 * T->nVec * T->stride;
    MUGIQ_REQUIRE(T->parity_offset >= unit && T->parity_offset % unit == 0 && T->parity_offset / unit <= kBoMaxNV,
                  "%s: a coarse -> coarse V must have parity_offset = 2 nColor n_vec stride with nColor in [1, %d] (it is %lld, 2 n_vec stride = %lld)", who,
                  kBoMaxNV, (long long)T->parity_offset, (long long)unit);
    L.K = (int)(T->parity_offset / unit);
  }
  L.m = L.K * L.g.aggVol;
  L.nBlocks = 2 * 2 * L.g.volumeCBc;
  MUGIQ_REQUIRE(T->nVec <= L.m, "%s: n_vec = %d columns cannot be orthonormal in blocks of m = %d rows", who, T->nVec, L.m);
  L.ldsBytes = (size_t)L.m * (sizeof(Z) + sizeof(int64_t));
  if (L.ldsBytes > kTransferMaxLds - 4096)
    return set_error(MUGIQ_HIP_ERROR_UNSUPPORTED, "%s: a column of m = %d rows (%zu bytes with the row table) does not fit the LDS of a workgroup", who, L.m,
                     L.ldsBytes);
  *out = L;
  return MUGIQ_HIP_SUCCESS;
}

BoArgs bo_args(const MugiqHipTransfer *T, const BoLevel &L, int nPasses) {
  BoArgs A{};
  A.V = const_cast<void *>(T->V);
  A.po = T->parity_offset;
  A.stride = T->stride, A.nVec = T->nVec;
  for (int d = 0; d < 4; d++) A.X[d] = L.g.X[d], A.Xc[d] = L.g.Xc[d], A.bs[d] = L.g.bs[d];
  A.aggVol = L.g.aggVol, A.K = L.K, A.m = L.m, A.nPasses = nPasses;
  return A;
}

template <typename Kernel> int bo_launch(Kernel kern, const BoLevel &L, const BoArgs &A, hipStream_t s) {
  return launch_with_lds(kern, dim3((unsigned)L.nBlocks), kBoThreads, L.ldsBytes, s, A);
}

// the per-block outputs in the stream's workspace: [ratio | dev | zeros | result]
struct BoScratch {
  double *ratio, *dev;
  int *zeros;
  BoResult *result;
};
int bo_scratch(BoScratch *out, int nBlocks, hipStream_t s) {
  void *ws = nullptr;
  const size_t n = (size_t)nBlocks;
  if (int st = stream_workspace(&ws, align256(8 * n) * 2 + align256(4 * n) + 256, s)) return st;
  unsigned char *cur = static_cast<unsigned char *>(ws);
  out->ratio = reinterpret_cast<double *>(cur);
  cur += align256(8 * n);
  out->dev = reinterpret_cast<double *>(cur);
  cur += align256(8 * n);
  out->zeros = reinterpret_cast<int *>(cur);
  cur += align256(4 * n);
  out->result = reinterpret_cast<BoResult *>(cur);
  return MUGIQ_HIP_SUCCESS;
}
int bo_fetch(BoResult *host, const BoScratch &sc, bool ortho, int nBlocks, hipStream_t s) {
  hipLaunchKernelGGL(block_info_kernel, dim3(1), dim3(kBoThreads), 0, s, ortho ? sc.ratio : (const double *)nullptr, ortho ? sc.zeros : (const int *)nullptr,
                     ortho ? (const double *)nullptr : sc.dev, nBlocks, sc.result);
  MUGIQ_CHECK_HIP(hipGetLastError());
  MUGIQ_CHECK_HIP(hipMemcpyAsync(host, sc.result, sizeof(BoResult), hipMemcpyDeviceToHost, s));
  MUGIQ_CHECK_HIP(hipStreamSynchronize(s));
  return MUGIQ_HIP_SUCCESS;
}

int check_ortho_param(int nPasses, double rankTol, const char *who) {
  MUGIQ_REQUIRE(nPasses >= 1 && nPasses <= 4, "%s: nPasses = %d must be in [1, 4]", who, nPasses);
  MUGIQ_REQUIRE(rankTol >= 0.0 && rankTol <= 1.0, "%s: rankTol = %g must be in [0, 1]", who, rankTol);
  return MUGIQ_HIP_SUCCESS;
}

int block_orthonormalize(const MugiqHipTransfer *T, const BoLevel &L, int nPasses, double rankTol, MugiqHipBlockOrthoInfo *info, hipStream_t s, const char *who) {
  BoScratch sc;
  if (int st = bo_scratch(&sc, L.nBlocks, s)) return st;
  BoArgs A = bo_args(T, L, nPasses);
  A.blockRatio = sc.ratio, A.blockZeros = sc.zeros;
  if (int st = T->precision == 8 ? bo_launch(block_ortho_kernel<double>, L, A, s) : bo_launch(block_ortho_kernel<float>, L, A, s)) return st;
  BoResult res;
  if (int st = bo_fetch(&res, sc, true, L.nBlocks, s)) return st;
  if (info) {
    info->minPivotRatio = res.minRatio;
    info->zeroColumns = (int)res.zeros;
  }
  if (!(res.minRatio >= rankTol) && rankTol > 0.0)
    return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT,
                     "%s: a column kept only %.3e of its norm against the columns before it (rankTol = %.3e): the vectors are dependent in some block "
                     "(V and info are filled)", who, res.minRatio, rankTol);
  return MUGIQ_HIP_SUCCESS;
}

int transfer_orthonormality(const MugiqHipTransfer *T, const BoLevel &L, double *out, hipStream_t s) {
  BoScratch sc;
  if (int st = bo_scratch(&sc, L.nBlocks, s)) return st;
  BoArgs A = bo_args(T, L, 0);
  A.blockDev = sc.dev;
  if (int st = T->precision == 8 ? bo_launch(ortho_check_kernel<double>, L, A, s) : bo_launch(ortho_check_kernel<float>, L, A, s)) return st;
  BoResult res;
  if (int st = bo_fetch(&res, sc, false, L.nBlocks, s)) return st;
  *out = res.maxDev;
  return MUGIQ_HIP_SUCCESS;
}

// a finest-level transfer and fine vectors on its lattice
int check_pack(const MugiqHipTransfer *T, const MugiqHipSpinorField *v, int n, const char *who, BoLevel *L) {
  MUGIQ_REQUIRE(T != nullptr && v != nullptr, "%s: NULL argument", who);
  if (int st = bo_level(T, who, L)) return st;
  MUGIQ_REQUIRE(T->spinBlockSize == 2, "%s: a finest-level transfer (spin_block_size 2) is needed, this one has %d", who, T->spinBlockSize);
  for (int i = 0; i < n; i++) {
    if (int st = validate_spinor(&v[i], who, "vector")) return st;
    MUGIQ_REQUIRE(same_geometry(v[i], v[0]), "%s: vector %d differs in precision, field order or geometry from vector 0", who, i);
  }
  for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(v[0].X[d] == T->X[d], "%s: the vectors have X[%d] = %d, the transfer %d", who, d, v[0].X[d], T->X[d]);
  return MUGIQ_HIP_SUCCESS;
}

// vectors of precision sPrec and field order `order` into V of precision vPrec (pack: A.vecs), or column A.j of V into A.vec
int launch_pack(bool pack, int vPrec, int sPrec, int order, const PackArgs &A, hipStream_t s) {
  with_storage(vPrec, sPrec, [&](auto fv, auto fs) {
    using FV = decltype(fv);
    using FS = decltype(fs);
    const auto kern = pack ? (order == 2 ? pack_vectors_kernel<FV, FS, 2> : pack_vectors_kernel<FV, FS, 4>)
                           : (order == 2 ? unpack_vector_kernel<FV, FS, 2> : unpack_vector_kernel<FV, FS, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)((A.volumeCB + 255) / 256), 12, 2), dim3(256), 0, s, A);
  });
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

PackArgs pack_args(const MugiqHipTransfer *T, const MugiqHipSpinorField &v) {
  PackArgs A{};
  A.V = const_cast<void *>(T->V);
  A.po = T->parity_offset;
  A.stride = T->stride, A.nVec = T->nVec, A.volumeCB = v.volumeCB;
  A.vStride = v.stride, A.vPo = v.parity_offset;
  return A;
}

int set_vectors(const MugiqHipTransfer *T, const MugiqHipSpinorField *v, hipStream_t s) {
  std::vector<const void *> host(T->nVec);
  for (int j = 0; j < T->nVec; j++) host[j] = v[j].data;
  void *table = nullptr;
  if (int st = upload_table(&table, host.data(), sizeof(void *) * host.size(), s)) return st;
  PackArgs A = pack_args(T, v[0]);
  A.vecs = static_cast<const void *const *>(table);
  return launch_pack(true, T->precision, v[0].precision, v[0].field_order, A, s);
}

int field_sub(const MugiqHipSpinorField &dst, const MugiqHipSpinorField &a, const MugiqHipSpinorField &b, hipStream_t s) {
  SubArgs A{};
  A.dst = static_cast<Z *>(dst.data), A.a = static_cast<const Z *>(a.data), A.b = static_cast<const Z *>(b.data);
  const bool f2 = dst.field_order == 2;
  A.nRows = f2 ? 12 : 6;
  A.rowLen = f2 ? dst.volumeCB : (int64_t)2 * dst.volumeCB;
  A.rowStride = f2 ? dst.stride : (int64_t)2 * dst.stride;
  A.po = dst.parity_offset;
  const int64_t total = 2 * A.nRows * A.rowLen;
  hipLaunchKernelGGL(field_sub_kernel, dim3((unsigned)std::min<int64_t>(4096, (total + 255) / 256)), dim3(256), 0, s, A);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

struct DeviceSlab {
  void *p = nullptr;
  ~DeviceSlab() {
    if (p) (void)hipFree(p);
  }
};

int check_setup_param(const MugiqHipMgSetupParam *p, const char *who) {
  MUGIQ_REQUIRE(p->setupMaxIter >= 0 && p->setupTol > 0.0, "%s: setupMaxIter = %d must be non-negative and setupTol = %g positive", who, p->setupMaxIter,
                p->setupTol);
  if (int st = check_ortho_param(p->nBlockOrtho, p->rankTol, who)) return st;
  MUGIQ_REQUIRE(p->refineCycles >= 0 && p->refineCycles <= 16, "%s: refineCycles = %d must be in [0, 16]", who, p->refineCycles);
  MUGIQ_REQUIRE(p->refineIters >= 1 && p->refineIters <= 16, "%s: refineIters = %d must be in [1, 16]", who, p->refineIters);
  return MUGIQ_HIP_SUCCESS;
}

}  // namespace
}  // namespace mugiq

using namespace mugiq;

extern "C" {

int mugiq_hip_block_orthonormalize(const MugiqHipTransfer *transfer, int nPasses, double rankTol, MugiqHipBlockOrthoInfo *info, void *stream) {
  const char *who = "blockOrthonormalize";
  BoLevel L;
  int st;
  if ((st = bo_level(transfer, who, &L))) return st;
  if ((st = check_ortho_param(nPasses, rankTol, who))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  return block_orthonormalize(transfer, L, nPasses, rankTol, info, s, who);
}

int mugiq_hip_transfer_orthonormality(const MugiqHipTransfer *transfer, double *out, void *stream) {
  const char *who = "transferOrthonormality";
  MUGIQ_REQUIRE(out != nullptr, "%s: out is NULL", who);
  BoLevel L;
  int st;
  if ((st = bo_level(transfer, who, &L))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  return transfer_orthonormality(transfer, L, out, s);
}

int mugiq_hip_transfer_set_vectors(const MugiqHipTransfer *transfer, const MugiqHipSpinorField *vecs_h, int nVec, void *stream) {
  const char *who = "transferSetVectors";
  BoLevel L;
  MUGIQ_REQUIRE(transfer != nullptr && vecs_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nVec == transfer->nVec, "%s: %d vectors for a transfer of n_vec = %d", who, nVec, transfer->nVec);
  if (int st = check_pack(transfer, vecs_h, nVec, who, &L)) return st;
  return set_vectors(transfer, vecs_h, static_cast<hipStream_t>(stream));
}

int mugiq_hip_transfer_get_vector(const MugiqHipSpinorField *vec, const MugiqHipTransfer *transfer, int j, void *stream) {
  const char *who = "transferGetVector";
  BoLevel L;
  if (int st = check_pack(transfer, vec, 1, who, &L)) return st;
  MUGIQ_REQUIRE(j >= 0 && j < transfer->nVec, "%s: j = %d is not in [0, n_vec = %d)", who, j, transfer->nVec);
  PackArgs A = pack_args(transfer, *vec);
  A.vec = vec->data, A.j = j;
  return launch_pack(false, transfer->precision, vec->precision, vec->field_order, A, static_cast<hipStream_t>(stream));
}

int mugiq_hip_mg_setup_param_default(MugiqHipMgSetupParam *p) {
  MUGIQ_REQUIRE(p != nullptr, "mgSetupParamDefault: param is NULL");
  p->setupMaxIter = 500;  // tests/loop.cpp:350
  p->setupTol = 5e-6;     // tests/loop.cpp:349
  p->nBlockOrtho = 2;
  p->rankTol = 1e-8;
  p->refineCycles = 0;
  p->refineIters = 4;
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_mg_setup(const MugiqHipTransfer *transfer, MugiqHipCoarseOperator *coarseOp, const MugiqHipSpinorField *start_h, int nVec,
                       const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover, double kappa, const MugiqHipMgSetupParam *p,
                       MugiqHipMgSetupInfo *info, const MugiqHipComm *comm, void *stream) {
  const char *who = "mgSetup";
  MUGIQ_REQUIRE(transfer != nullptr && start_h != nullptr && gauge != nullptr && p != nullptr && info != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nVec >= 1, "%s: nVec = %d must be >= 1", who, nVec);
  int st;
  if ((st = check_setup_param(p, who))) return st;
  if ((st = check_single_domain(comm, who))) return st;
  BoLevel L;
  if ((st = check_pack(transfer, start_h, nVec, who, &L))) return st;
  MUGIQ_REQUIRE(nVec == transfer->nVec && nVec <= kSetupMaxNV, "%s: %d start vectors for a transfer of n_vec = %d", who, nVec, transfer->nVec);
  MUGIQ_REQUIRE(start_h[0].precision == 8, "%s: the start vectors have precision %d: the setup solves run in fp64", who, start_h[0].precision);
  const int part[4] = {0, 0, 0, 0};
  if ((st = check_gauge(gauge, start_h[0].X, part, who))) return st;
  if (clover) {
    if ((st = validate_clover(clover, start_h[0].X, start_h[0].volumeCB, who))) return st;
    MUGIQ_REQUIRE(clover->precision == gauge->precision, "%s: clover precision %d differs from the gauge precision %d", who, clover->precision, gauge->precision);
  }
  MUGIQ_REQUIRE(p->refineCycles == 0 || coarseOp != nullptr, "%s: refineCycles = %d needs a coarse operator to refine with", who, p->refineCycles);
  if (coarseOp) {
    if ((st = validate_coarse_operator(coarseOp, who))) return st;
    MUGIQ_REQUIRE(coarseOp->nVec == nVec && coarseOp->precision == transfer->precision, "%s: the coarse operator has n_vec %d and precision %d, the transfer %d and %d",
                  who, coarseOp->nVec, coarseOp->precision, nVec, transfer->precision);
    for (int d = 0; d < 4; d++)
      MUGIQ_REQUIRE(coarseOp->X[d] == L.g.Xc[d], "%s: coarse operator X[%d] = %d, the transfer's coarse lattice has %d", who, d, coarseOp->X[d], L.g.Xc[d]);
  }
  if (p->refineCycles > 0 && transfer->precision != 8)
    return set_error(MUGIQ_HIP_ERROR_UNSUPPORTED, "%s: refinement runs the two-grid solve, which is fp64 only: the transfer has precision %d", who, transfer->precision);

  hipStream_t s = static_cast<hipStream_t>(stream);
  *info = MugiqHipMgSetupInfo{};
  // the null vectors and two blocks of work vectors, laid out like the start vectors; not from the per-stream arenas, which the operator,
  // the solvers and the coarse-operator build below take for themselves
  const size_t fb = align256((size_t)2 * (size_t)start_h[0].parity_offset * sizeof(Z));
  DeviceSlab slab;
  if (hipMalloc(&slab.p, fb * (size_t)(nVec + 2 * kSetupBlock)) != hipSuccess) {
    slab.p = nullptr;
    return set_error(MUGIQ_HIP_ERROR_HIP, "%s: no device memory for %d work vectors of %zu bytes", who, nVec + 2 * kSetupBlock, fb);
  }
  MUGIQ_CHECK_HIP(hipMemsetAsync(slab.p, 0, fb * (size_t)(nVec + 2 * kSetupBlock), s));
  std::vector<MugiqHipSpinorField> v(nVec);
  MugiqHipSpinorField rhs[kSetupBlock], sol[kSetupBlock];
  auto carve = [&](int k) {
    MugiqHipSpinorField f = start_h[0];
    f.data = static_cast<unsigned char *>(slab.p) + fb * (size_t)k;
    for (int d = 0; d < 4; d++) f.ghost[d][0] = f.ghost[d][1] = nullptr;
    return f;
  };
  for (int j = 0; j < nVec; j++) v[j] = carve(j);
  for (int i = 0; i < kSetupBlock; i++) rhs[i] = carve(nVec + i), sol[i] = carve(nVec + kSetupBlock + i);

  int reads = 0, cgReads = 0;  // counted; and what the CG, which does not count, makes by its source
  // null vector j: b = M start_j, e = CG(b) stopped early, v_j = start_j - e
  for (int v0 = 0; v0 < nVec; v0 += kSetupBlock) {
    const int n = std::min(kSetupBlock, nVec - v0);
    if ((st = mugiq_hip_wilson_clover_apply(rhs, start_h + v0, n, gauge, clover, kappa, MUGIQ_HIP_EIG_OPERATOR_M, 1.0, nullptr, stream))) return st;
    double relres[kSetupBlock];
    st = mugiq_hip_wilson_clover_solve(sol, rhs, n, gauge, clover, kappa, nullptr, nullptr, 0, p->setupTol, p->setupMaxIter, info->cgIters + v0, relres, nullptr, stream);
    if (st != MUGIQ_HIP_SUCCESS && st != MUGIQ_HIP_ERROR_NOT_CONVERGED) return st;
    cgReads += 2 * *std::max_element(info->cgIters + v0, info->cgIters + v0 + n) + 3;  // two per iteration, three per block (csrc/wilson.hip)
    for (int i = 0; i < n; i++)
      if ((st = field_sub(v[v0 + i], start_h[v0 + i], sol[i], s))) return st;
  }
  MugiqHipBlockOrthoInfo bo{};
  int rank = MUGIQ_HIP_SUCCESS;
  auto finish = [&]() -> int {  // V from the vectors, block-orthonormal, and its coarse operator
    int e;
    if ((e = set_vectors(transfer, v.data(), s))) return e;
    if ((e = debug_poison_lds_if_asked(s))) return e;
    rank = block_orthonormalize(transfer, L, p->nBlockOrtho, p->rankTol, &bo, s, who);
    reads++;
    if (rank != MUGIQ_HIP_SUCCESS && rank != MUGIQ_HIP_ERROR_INVALID_ARGUMENT) return rank;
    if (coarseOp && (e = mugiq_hip_compute_coarse_operator(coarseOp, transfer, gauge, clover, kappa, nullptr, stream))) return e;
    return MUGIQ_HIP_SUCCESS;
  };
  if ((st = finish())) return st;
  // adaptive refinement: v_j -= K-preconditioned GCR(M v_j), a few iterations on the hierarchy so far
  for (int cycle = 0; cycle < p->refineCycles && rank == MUGIQ_HIP_SUCCESS; cycle++) {
    MugiqHipMgSolveParam mp;
    mugiq_hip_mg_solve_param_default(&mp);
    mp.tol = p->setupTol, mp.maxIter = p->refineIters, mp.nKrylov = p->refineIters;
    for (int v0 = 0; v0 < nVec; v0 += kSetupBlock) {
      const int n = std::min(kSetupBlock, nVec - v0);
      if ((st = mugiq_hip_wilson_clover_apply(rhs, v.data() + v0, n, gauge, clover, kappa, MUGIQ_HIP_EIG_OPERATOR_M, 1.0, nullptr, stream))) return st;
      int iters[kSetupBlock], r = 0;
      double relres[kSetupBlock];
      st = mugiq_hip_mg_solve(sol, rhs, n, gauge, clover, kappa, transfer, coarseOp, &mp, iters, relres, nullptr, 0, &r, nullptr, stream);
      if (st != MUGIQ_HIP_SUCCESS && st != MUGIQ_HIP_ERROR_NOT_CONVERGED) return st;
      reads += r;
      for (int i = 0; i < n; i++)
        if ((st = field_sub(v[v0 + i], v[v0 + i], sol[i], s))) return st;
    }
    if ((st = finish())) return st;
  }
  if ((st = transfer_orthonormality(transfer, L, &info->orthonormality, s))) return st;
  reads++;
  info->minPivotRatio = bo.minPivotRatio;
  info->zeroColumns = bo.zeroColumns;
  info->hostReads = reads;
  info->cgHostReadsEstimate = cgReads;
  MUGIQ_CHECK_HIP(hipStreamSynchronize(s));
  if (rank != MUGIQ_HIP_SUCCESS)
    return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: the null vectors are dependent in some block: minPivotRatio = %.3e < rankTol = %.3e (V and info are filled)",
                     who, bo.minPivotRatio, p->rankTol);
  return MUGIQ_HIP_SUCCESS;
}

}  // extern "C"
