// The clover term of the Wilson-clover operator: the field type (alloc / free / bytes) and the kernel that builds it from the
// border-extended gauge field.  Definition and packed element order: MugiqHipCloverField in include/mugiq_hip.h.
//
//   A(x) = 1 + i coeff sum_{m<n} sigma_mn (x) Fhat_mn(x),   sigma_mn = (i/2) [g_m, g_n] = i g_m g_n,   Fhat_mn = (Q_mn - Q_mn^dag) / 8
//
// g5 = diag(1, 1, -1, -1) is diagonal, so every sigma_mn has one entry per row and stays inside the spin pairs (0, 1) and (2, 3): A is two
// Hermitian 6 x 6 blocks.  Fhat is anti-Hermitian to the bit (each entry is a difference and its negated conjugate), so A is Hermitian
// to the bit and the strictly-lower triangle plus the real diagonal hold all of it.
//
// clover_kernel: one lattice site per lane, the six planes one after the other, each with its four leaves (three 3 x 3 products per leaf,
// 16 link loads per plane).  Links come from the extended field as the stencil's do (wilson_hop in wilson.hip): x +- m across a face is
// in the border where R >= 1 and wraps where R = 0; the diagonal neighbours x - m + n, x + m - n, x - m - n are in its edges and corners.
// fp64 arithmetic whatever the storage; the 72 reals of a site are rounded once, on the store.
#include "internal.h"

namespace mugiq {
namespace {

constexpr int kCloverThreads = 128;
constexpr int kCloverGamma[4] = {1, 2, 4, 8};

struct CloverGeom {
  int X[4], XE[4], brd[4];
  int volumeCB, stride, gstride;
  int64_t po, gpo;  // parity offsets (complex elements) of the clover field and of the gauge field
};

typedef Cplx<double> C64;

// w = a b | a b^dag | a^dag b
__device__ inline void mul_nn(C64 w[9], const C64 a[9], const C64 b[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      C64 t{0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 3; k++) cmadd(t, a[i * 3 + k], b[k * 3 + j]);
      w[i * 3 + j] = t;
    }
}
__device__ inline void mul_nd(C64 w[9], const C64 a[9], const C64 b[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      C64 t{0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 3; k++) cmadd(t, a[i * 3 + k], C64{b[j * 3 + k].re, -b[j * 3 + k].im});
      w[i * 3 + j] = t;
    }
}
__device__ inline void mul_dn(C64 w[9], const C64 a[9], const C64 b[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      C64 t{0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 3; k++) cmadd_conj(t, a[k * 3 + i], b[k * 3 + j]);
      w[i * 3 + j] = t;
    }
}

// U_dir(x + sm m + sn n) from the extended field; c2: the extended coordinates of x, pty: the parity of x
template <typename FG, int M, int N>
__device__ inline void load_link(C64 u[9], const FG *U, const CloverGeom &g, const int c2[4], int pty, int dir, int sm, int sn) {
  typedef FG gvec2 __attribute__((ext_vector_type(2)));
  int dx[4] = {0, 0, 0, 0};
  dx[M] = sm;
  dx[N] = sn;
  const int lp = (pty + sm + sn) & 1;
  const int lidx = link_index_shift(c2, dx, g.XE);
  const MUGIQ_GLOBAL gvec2 *p = as_global(reinterpret_cast<const gvec2 *>(U)) + lp * g.gpo + (int64_t)dir * 9 * g.gstride + lidx;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const gvec2 t = p[(int64_t)i * g.gstride];
    u[i] = C64{(double)t.x, (double)t.y};
  }
}

// index of entry (i, j), i > j, of a 6 x 6 block among its 15 strictly-lower ones
__device__ constexpr int lower_index(int i, int j) { return i * (i - 1) / 2 + j; }

// diag / low += i coeff sigma_MN (x) F, the entries on and below the diagonal
template <int M, int N> __device__ inline void add_plane(double diag[2][6], C64 low[2][15], const C64 F[9], double coeff) {
  constexpr int GM = kCloverGamma[M], GN = kCloverGamma[N];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    // (g_M g_N)_{s, t} = i^(phM[s] + phN[cM]) delta(t, colN[cM]), cM = colM[s];  i coeff sigma = i coeff i g_M g_N = -coeff g_M g_N
    const int cM = kGammaColumn[GM][s];
    const int t = kGammaColumn[GN][cM];
    const int ph = (kGammaPhase[GM][s] + kGammaPhase[GN][cM] + 2) & 3;
    const int b = s >> 1, sl = s & 1, tl = t & 1;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int row = sl * 3 + a, col = tl * 3 + c;
        if (row < col) continue;
        C64 z{0.0, 0.0};
        add_phase(z, ph, F[a * 3 + c]);
        if (row == col) diag[b][row] = fma(coeff, z.re, diag[b][row]);
        else {
          low[b][lower_index(row, col)].re = fma(coeff, z.re, low[b][lower_index(row, col)].re);
          low[b][lower_index(row, col)].im = fma(coeff, z.im, low[b][lower_index(row, col)].im);
        }
      }
  }
}

template <typename FG, int M, int N>
__device__ inline void clover_plane(double diag[2][6], C64 low[2][15], const FG *U, const CloverGeom &g, const int c2[4], int pty, double coeff) {
  C64 Q[9], a[9], b[9], w[9], w2[9];
  // U_m(x) U_n(x+m) U_m^dag(x+n) U_n^dag(x)
  load_link<FG, M, N>(a, U, g, c2, pty, M, 0, 0);
  load_link<FG, M, N>(b, U, g, c2, pty, N, 1, 0);
  mul_nn(w, a, b);
  load_link<FG, M, N>(a, U, g, c2, pty, M, 0, 1);
  mul_nd(w2, w, a);
  load_link<FG, M, N>(a, U, g, c2, pty, N, 0, 0);
  mul_nd(Q, w2, a);
  // U_n(x) U_m^dag(x-m+n) U_n^dag(x-m) U_m(x-m)
  load_link<FG, M, N>(b, U, g, c2, pty, M, -1, 1);
  mul_nd(w, a, b);
  load_link<FG, M, N>(a, U, g, c2, pty, N, -1, 0);
  mul_nd(w2, w, a);
  load_link<FG, M, N>(a, U, g, c2, pty, M, -1, 0);
  mul_nn(w, w2, a);
#pragma unroll
  for (int i = 0; i < 9; i++) Q[i] = C64{Q[i].re + w[i].re, Q[i].im + w[i].im};
  // U_m^dag(x-m) U_n^dag(x-m-n) U_m(x-m-n) U_n(x-n)
  load_link<FG, M, N>(b, U, g, c2, pty, N, -1, -1);
  mul_nn(w, b, a);  // U_n(x-m-n) U_m(x-m), daggered below
  load_link<FG, M, N>(a, U, g, c2, pty, M, -1, -1);
  mul_dn(w2, w, a);
  load_link<FG, M, N>(a, U, g, c2, pty, N, 0, -1);
  mul_nn(w, w2, a);
#pragma unroll
  for (int i = 0; i < 9; i++) Q[i] = C64{Q[i].re + w[i].re, Q[i].im + w[i].im};
  // U_n^dag(x-n) U_m(x-n) U_n(x+m-n) U_m^dag(x)
  load_link<FG, M, N>(b, U, g, c2, pty, M, 0, -1);
  mul_dn(w, a, b);
  load_link<FG, M, N>(a, U, g, c2, pty, N, 1, -1);
  mul_nn(w2, w, a);
  load_link<FG, M, N>(a, U, g, c2, pty, M, 0, 0);
  mul_nd(w, w2, a);
#pragma unroll
  for (int i = 0; i < 9; i++) Q[i] = C64{Q[i].re + w[i].re, Q[i].im + w[i].im};
  C64 F[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) F[i * 3 + j] = C64{0.125 * (Q[i * 3 + j].re - Q[j * 3 + i].re), 0.125 * (Q[i * 3 + j].im + Q[j * 3 + i].im)};
  add_plane<M, N>(diag, low, F, coeff);
}

template <typename FC, typename FG>
__global__ __launch_bounds__(kCloverThreads) void clover_kernel(FC *clover, const FG *U, CloverGeom g, double coeff) {
  typedef FC cvec2 __attribute__((ext_vector_type(2)));
  const int site = blockIdx.x * kCloverThreads + threadIdx.x;
  if (site >= 2 * g.volumeCB) return;
  const int pty = site >= g.volumeCB ? 1 : 0;
  const int x_cb = site - pty * g.volumeCB;
  int coord[4], c2[4];
  get_coords(coord, x_cb, g.X, pty);
#pragma unroll
  for (int i = 0; i < 4; i++) c2[i] = coord[i] + g.brd[i];
  double diag[2][6];
  C64 low[2][15];
#pragma unroll
  for (int b = 0; b < 2; b++) {
#pragma unroll
    for (int i = 0; i < 6; i++) diag[b][i] = 1.0;
#pragma unroll
    for (int i = 0; i < 15; i++) low[b][i] = C64{0.0, 0.0};
  }
  // one plane at a time: without the barriers the scheduler hoists the 96 link loads of all six planes to the front and spills
  clover_plane<FG, 0, 1>(diag, low, U, g, c2, pty, coeff);
  __builtin_amdgcn_sched_barrier(0);
  clover_plane<FG, 0, 2>(diag, low, U, g, c2, pty, coeff);
  __builtin_amdgcn_sched_barrier(0);
  clover_plane<FG, 0, 3>(diag, low, U, g, c2, pty, coeff);
  __builtin_amdgcn_sched_barrier(0);
  clover_plane<FG, 1, 2>(diag, low, U, g, c2, pty, coeff);
  __builtin_amdgcn_sched_barrier(0);
  clover_plane<FG, 1, 3>(diag, low, U, g, c2, pty, coeff);
  __builtin_amdgcn_sched_barrier(0);
  clover_plane<FG, 2, 3>(diag, low, U, g, c2, pty, coeff);
  MUGIQ_GLOBAL cvec2 *p = as_global(reinterpret_cast<cvec2 *>(clover)) + pty * g.po + x_cb;
#pragma unroll
  for (int b = 0; b < 2; b++) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
      cvec2 t;
      t.x = (FC)diag[b][2 * q];
      t.y = (FC)diag[b][2 * q + 1];
      p[(int64_t)(b * 18 + q) * g.stride] = t;
    }
#pragma unroll
    for (int l = 0; l < 15; l++) {
      cvec2 t;
      t.x = (FC)low[b][l].re;
      t.y = (FC)low[b][l].im;
      p[(int64_t)(b * 18 + 3 + l) * g.stride] = t;
    }
  }
}

}  // namespace

int validate_clover(const MugiqHipCloverField *C, const int X[4], int volumeCB, const char *who) {
  MUGIQ_REQUIRE(C != nullptr && C->data != nullptr, "%s: clover field is NULL", who);
  MUGIQ_REQUIRE(C->precision == 4 || C->precision == 8, "%s: clover precision %d", who, C->precision);
  long long vol = 1;
  for (int d = 0; d < 4; d++) {
    MUGIQ_REQUIRE(C->X[d] > 0 && (C->X[d] & 1) == 0, "%s: clover X[%d] = %d must be positive and even", who, d, C->X[d]);
    MUGIQ_REQUIRE(X == nullptr || C->X[d] == X[d], "%s: clover X[%d] = %d differs from the field's %d", who, d, C->X[d], X ? X[d] : 0);
    vol *= C->X[d];
  }
  MUGIQ_REQUIRE(vol / 2 < (1LL << 30), "%s: clover volume overflows int", who);
  MUGIQ_REQUIRE(C->volumeCB == (int)(vol / 2) && (X == nullptr || C->volumeCB == volumeCB), "%s: clover volumeCB %d is not half the volume %lld", who,
                C->volumeCB, vol);
  MUGIQ_REQUIRE(C->stride >= C->volumeCB, "%s: clover stride %d < volumeCB %d", who, C->stride, C->volumeCB);
  MUGIQ_REQUIRE(C->parity_offset >= (int64_t)36 * C->stride, "%s: clover parity_offset %lld < 36*stride", who, (long long)C->parity_offset);
  return MUGIQ_HIP_SUCCESS;
}

}  // namespace mugiq

using namespace mugiq;

extern "C" {

size_t mugiq_hip_clover_bytes(const int X[4], int precision) {
  if (!X || (precision != 4 && precision != 8)) return 0;
  size_t vol = 1;
  for (int d = 0; d < 4; d++) vol *= (size_t)X[d];
  return vol / 2 * 36 * 2 * 2 * (size_t)precision;  // volumeCB * 36 pairs * 2 parities * 2 reals
}

int mugiq_hip_alloc_clover(MugiqHipCloverField *clover, const int X[4], int precision) {
  const char *who = "allocClover";
  MUGIQ_REQUIRE(clover && X, "%s: NULL argument", who);
  MUGIQ_REQUIRE(precision == 4 || precision == 8, "%s: precision %d", who, precision);
  long long vol = 1;
  for (int d = 0; d < 4; d++) {
    MUGIQ_REQUIRE(X[d] > 0 && (X[d] & 1) == 0, "%s: X[%d] = %d must be positive and even", who, d, X[d]);
    clover->X[d] = X[d];
    vol *= X[d];
  }
  MUGIQ_REQUIRE(vol / 2 < (1LL << 30), "%s: volume overflows int", who);
  clover->precision = precision;
  clover->volumeCB = clover->stride = (int)(vol / 2);
  clover->parity_offset = (int64_t)36 * clover->stride;
  clover->data = nullptr;
  const size_t bytes = mugiq_hip_clover_bytes(X, precision);
  MUGIQ_CHECK_HIP(hipMalloc(&clover->data, bytes));
  MUGIQ_CHECK_HIP(hipMemset(clover->data, 0, bytes));
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_free_clover(MugiqHipCloverField *clover) {
  if (clover && clover->data) {
    MUGIQ_CHECK_HIP(hipFree(clover->data));
    clover->data = nullptr;
  }
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_compute_clover(const MugiqHipCloverField *clover, const MugiqHipGaugeField *gauge, double coeff, const MugiqHipComm *comm,
                             void *stream) {
  const char *who = "computeClover";
  int st, part[4];
  if ((st = validate_clover(clover, nullptr, 0, who))) return st;
  if ((st = check_comm(comm, part, false, who))) return st;
  if ((st = check_gauge(gauge, clover->X, part, who))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  CloverGeom g;
  for (int d = 0; d < 4; d++) {
    g.X[d] = clover->X[d];
    g.brd[d] = gauge->R[d];
    g.XE[d] = clover->X[d] + 2 * gauge->R[d];
  }
  g.volumeCB = clover->volumeCB;
  g.stride = clover->stride;
  g.po = clover->parity_offset;
  g.gstride = gauge->stride;
  g.gpo = gauge->parity_offset;
  const dim3 grid((2 * clover->volumeCB + kCloverThreads - 1) / kCloverThreads), block(kCloverThreads);
  if (clover->precision == 8 && gauge->precision == 8)
    hipLaunchKernelGGL((clover_kernel<double, double>), grid, block, 0, s, static_cast<double *>(clover->data), static_cast<const double *>(gauge->data), g, coeff);
  else if (clover->precision == 8)
    hipLaunchKernelGGL((clover_kernel<double, float>), grid, block, 0, s, static_cast<double *>(clover->data), static_cast<const float *>(gauge->data), g, coeff);
  else if (gauge->precision == 8)
    hipLaunchKernelGGL((clover_kernel<float, double>), grid, block, 0, s, static_cast<float *>(clover->data), static_cast<const double *>(gauge->data), g, coeff);
  else
    hipLaunchKernelGGL((clover_kernel<float, float>), grid, block, 0, s, static_cast<float *>(clover->data), static_cast<const float *>(gauge->data), g, coeff);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

}  // extern "C"
