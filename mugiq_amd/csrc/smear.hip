// Stout smearing (Morningstar-Peardon) of the border-extended gauge field, the device-side border refresh and the plaquette.
// Definitions: the smearing block of include/mugiq_hip.h.
//
//   C_mu(x) = sum_{nu in S, nu != mu} [ U_nu(x) U_mu(x+nu) U_nu^dag(x+mu) + U_nu^dag(x-nu) U_mu(x-nu) U_nu(x-nu+mu) ]
//   Omega = rho C_mu(x) U_mu^dag(x),   Q = (i/2)(Omega^dag - Omega) - (i/6) tr(Omega^dag - Omega),   U'_mu(x) = exp(iQ) U_mu(x)
//
// stout_kernel: one link (mu, local site) per lane, mu = blockIdx.y (uniform over the workgroup, so the directions are compile-time
// inside every branch and no register array is indexed at run time).  Per other direction nu: the upper and the lower staple, six link
// loads and four 3 x 3 products, one staple at a time.  Links come from the extended field as clover.hip's do: x +- nu across a face is
// in the border where R >= 1 and wraps where R = 0; x - nu + mu is in the edge regions.  fp64 arithmetic whatever the storage; the 18
// reals of the new link are rounded once, on the store.  exp(iQ) by Cayley-Hamilton, f0 + f1 Q + f2 Q^2.
//
// Border refresh: one dimension after the other, each slab over the full extended range of the other three, so that later dimensions
// carry the borders of the earlier ones and edges and corners are filled -- the order of gauge_setup.cpp, with copies only: the result
// is that of mugiq_hip_create_extended_gauge to the bit.
//
// Plaquette: one local site per lane, six planes, the fixed-order fp64 reduction of wilson.hip's scalars.
#include <algorithm>
#include <cmath>

#include "internal.h"

namespace mugiq {
namespace {

constexpr int kStoutThreads = 128;
constexpr int kCopyThreads = 256;
constexpr int kPlaqThreads = 256;
constexpr int kPlaqMaxGroups = 1024;  // workgroups of the reduction: the partial sums one thread adds up in workgroup order

struct SmearGeom {
  int X[4], XE[4], brd[4];
  int volumeCB;
  int istride, ostride;  // complex elements between the planes of the field read and of the field written
  int64_t ipo, opo;      // ... and between their parities
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

// U_dir(x + sm m + sn n) from the extended field read; c2: the extended coordinates of x, pty: the parity of x
template <typename FG, int M, int N>
__device__ inline void load_link(C64 u[9], const FG *U, const SmearGeom &g, const int c2[4], int pty, int dir, int sm, int sn) {
  typedef FG gvec2 __attribute__((ext_vector_type(2)));
  int dx[4] = {0, 0, 0, 0};
  dx[M] += sm;
  dx[N] += sn;
  const int lp = (pty + sm + sn) & 1;
  const int lidx = link_index_shift(c2, dx, g.XE);
  const MUGIQ_GLOBAL gvec2 *p = as_global(reinterpret_cast<const gvec2 *>(U)) + lp * g.ipo + (int64_t)dir * 9 * g.istride + lidx;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const gvec2 t = p[(int64_t)i * g.istride];
    u[i] = C64{(double)t.x, (double)t.y};
  }
}

// C += U_nu(x) U_mu(x+nu) U_nu^dag(x+mu) + U_nu^dag(x-nu) U_mu(x-nu) U_nu(x-nu+mu)
template <typename FG, int MU, int NU>
__device__ inline void add_staples(C64 C[9], const FG *U, const SmearGeom &g, const int c2[4], int pty) {
  C64 a[9], b[9], w[9], w2[9];
  load_link<FG, MU, NU>(a, U, g, c2, pty, NU, 0, 0);
  load_link<FG, MU, NU>(b, U, g, c2, pty, MU, 0, 1);
  mul_nn(w, a, b);
  load_link<FG, MU, NU>(a, U, g, c2, pty, NU, 1, 0);
  mul_nd(w2, w, a);
#pragma unroll
  for (int i = 0; i < 9; i++) C[i] = C64{C[i].re + w2[i].re, C[i].im + w2[i].im};
  __builtin_amdgcn_sched_barrier(0);
  load_link<FG, MU, NU>(a, U, g, c2, pty, NU, 0, -1);
  load_link<FG, MU, NU>(b, U, g, c2, pty, MU, 0, -1);
  mul_dn(w, a, b);
  load_link<FG, MU, NU>(a, U, g, c2, pty, NU, 1, -1);
  mul_nn(w2, w, a);
#pragma unroll
  for (int i = 0; i < 9; i++) C[i] = C64{C[i].re + w2[i].re, C[i].im + w2[i].im};
}

// E = exp(iQ), Q Hermitian and traceless: f0 + f1 Q + f2 Q^2 with the coefficients of Morningstar and Peardon (hep-lat/0311018, eqs.
// 23-34): c0 = det Q, c1 = tr Q^2 / 2, the (u, w, xi0(w)) form, the series of xi0 for small w, and c0 -> -c0 through f_j -> (-1)^j f_j^*.
// Where c1 <= 1e-14 (|Q| below 1.5e-7, Q^3 / 6 below 1e-21: far under the rounding of 1) -- Q = 0 among them, where the closed form
// is 0/0 -- the series 1 + iQ - Q^2 / 2 is the result to rounding.
__device__ inline void exp_iq(C64 E[9], const C64 Q[9]) {
  C64 Q2[9];
  mul_nn(Q2, Q, Q);
  const double c1 = 0.5 * (Q2[0].re + Q2[4].re + Q2[8].re);
  C64 f0, f1, f2;
  if (!(c1 > 1e-14)) {
    f0 = C64{1.0, 0.0};
    f1 = C64{0.0, 1.0};
    f2 = C64{-0.5, 0.0};
  } else {
    // det Q = tr Q^3 / 3 for a traceless matrix: the real part of the diagonal of Q^2 Q
    double tr3 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int k = 0; k < 3; k++) tr3 += Q2[i * 3 + k].re * Q[k * 3 + i].re - Q2[i * 3 + k].im * Q[k * 3 + i].im;
    const double c0 = tr3 / 3.0;
    const bool flip = c0 < 0.0;
    const double c0a = fabs(c0);
    const double c13 = c1 / 3.0;
    const double c0max = 2.0 * c13 * sqrt(c13);
    const double theta = acos(fmin(c0a / c0max, 1.0));
    const double u = sqrt(c13) * cos(theta / 3.0);
    const double w = sqrt(c1) * sin(theta / 3.0);
    const double u2 = u * u, w2 = w * w;
    double xi0;
    if (fabs(w) <= 0.05) xi0 = 1.0 - w2 / 6.0 * (1.0 - w2 / 20.0 * (1.0 - w2 / 42.0));
    else xi0 = sin(w) / w;
    const double cw = cos(w);
    double s2u, c2u, su, cu;
    sincos(2.0 * u, &s2u, &c2u);
    sincos(u, &su, &cu);
    // e^{2iu} = (c2u, s2u), e^{-iu} = (cu, -su)
    // h0 = (u^2 - w^2) e^{2iu} + e^{-iu} [8 u^2 cos w + 2 i u (3 u^2 + w^2) xi0]
    const double a0 = 8.0 * u2 * cw, b0 = 2.0 * u * (3.0 * u2 + w2) * xi0;
    C64 h0{(u2 - w2) * c2u + cu * a0 + su * b0, (u2 - w2) * s2u + cu * b0 - su * a0};
    // h1 = 2u e^{2iu} - e^{-iu} [2 u cos w - i (3 u^2 - w^2) xi0]
    const double a1 = 2.0 * u * cw, b1 = -(3.0 * u2 - w2) * xi0;
    C64 h1{2.0 * u * c2u - (cu * a1 + su * b1), 2.0 * u * s2u - (cu * b1 - su * a1)};
    // h2 = e^{2iu} - e^{-iu} [cos w + 3 i u xi0]
    const double a2 = cw, b2 = 3.0 * u * xi0;
    C64 h2{c2u - (cu * a2 + su * b2), s2u - (cu * b2 - su * a2)};
    const double inv = 1.0 / (9.0 * u2 - w2);
    f0 = C64{h0.re * inv, h0.im * inv};
    f1 = C64{h1.re * inv, h1.im * inv};
    f2 = C64{h2.re * inv, h2.im * inv};
    if (flip) {
      f0.im = -f0.im;
      f1.re = -f1.re;
      f2.im = -f2.im;
    }
  }
#pragma unroll
  for (int i = 0; i < 9; i++) {
    C64 t{0.0, 0.0};
    cmadd(t, f1, Q[i]);
    cmadd(t, f2, Q2[i]);
    E[i] = t;
  }
  E[0].re += f0.re, E[0].im += f0.im;
  E[4].re += f0.re, E[4].im += f0.im;
  E[8].re += f0.re, E[8].im += f0.im;
}

template <typename FG> __device__ inline void store_link(FG *out, const SmearGeom &g, const int c2[4], int pty, int dir, const C64 v[9]) {
  typedef FG gvec2 __attribute__((ext_vector_type(2)));
  const int lidx = lex_index(c2, g.XE) >> 1;
  MUGIQ_GLOBAL gvec2 *p = as_global(reinterpret_cast<gvec2 *>(out)) + pty * g.opo + (int64_t)dir * 9 * g.ostride + lidx;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    gvec2 t;
    t.x = (FG)v[i].re;
    t.y = (FG)v[i].im;
    p[(int64_t)i * g.ostride] = t;
  }
}

// the new link mu of the site: the staples of the other directions below DIMS, one after the other, then the exponential
template <typename FG, int DIMS, int MU>
__device__ inline void stout_link(FG *out, const FG *U, const SmearGeom &g, const int c2[4], int pty, double rho) {
  constexpr int N0 = MU == 0 ? 1 : 0;
  C64 C[9];
#pragma unroll
  for (int i = 0; i < 9; i++) C[i] = C64{0.0, 0.0};
  // one staple at a time: without the barriers the scheduler hoists the link loads of every staple to the front and spills
  if constexpr (MU != 0) {
    add_staples<FG, MU, 0>(C, U, g, c2, pty);
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (MU != 1) {
    add_staples<FG, MU, 1>(C, U, g, c2, pty);
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (MU != 2) {
    add_staples<FG, MU, 2>(C, U, g, c2, pty);
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (MU != 3 && DIMS == 4) {
    add_staples<FG, MU, 3>(C, U, g, c2, pty);
    __builtin_amdgcn_sched_barrier(0);
  }
  C64 u[9], Om[9], Q[9], E[9];
  load_link<FG, MU, N0>(u, U, g, c2, pty, MU, 0, 0);
  mul_nd(Om, C, u);
  // Q = (i/2)(Omega^dag - Omega) - (i/6) tr(Omega^dag - Omega), Omega = rho C U^dag
  const double tr = (Om[0].im + Om[4].im + Om[8].im) / 3.0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      if (i == j) Q[i * 3 + j] = C64{rho * (Om[i * 3 + i].im - tr), 0.0};
      else
        Q[i * 3 + j] = C64{0.5 * rho * (Om[j * 3 + i].im + Om[i * 3 + j].im), 0.5 * rho * (Om[j * 3 + i].re - Om[i * 3 + j].re)};
    }
  exp_iq(E, Q);
  mul_nn(Om, E, u);
  store_link<FG>(out, g, c2, pty, MU, Om);
}

template <typename FG, int DIMS>
__global__ __launch_bounds__(kStoutThreads) void stout_kernel(FG *out, const FG *U, SmearGeom g, double rho) {
  const int site = blockIdx.x * kStoutThreads + threadIdx.x;
  if (site >= 2 * g.volumeCB) return;
  const int pty = site >= g.volumeCB ? 1 : 0;
  const int x_cb = site - pty * g.volumeCB;
  int coord[4], c2[4];
  get_coords(coord, x_cb, g.X, pty);
#pragma unroll
  for (int i = 0; i < 4; i++) c2[i] = coord[i] + g.brd[i];
  switch (blockIdx.y) {
  case 0: stout_link<FG, DIMS, 0>(out, U, g, c2, pty, rho); break;
  case 1: stout_link<FG, DIMS, 1>(out, U, g, c2, pty, rho); break;
  case 2: stout_link<FG, DIMS, 2>(out, U, g, c2, pty, rho); break;
  default:
    if constexpr (DIMS == 4) stout_link<FG, DIMS, 3>(out, U, g, c2, pty, rho);
    else {  // the t links of a spatial smearing: copied as they are
      typedef FG gvec2 __attribute__((ext_vector_type(2)));
      const int lidx = lex_index(c2, g.XE) >> 1;
      const MUGIQ_GLOBAL gvec2 *p = as_global(reinterpret_cast<const gvec2 *>(U)) + pty * g.ipo + (int64_t)27 * g.istride + lidx;
      MUGIQ_GLOBAL gvec2 *q = as_global(reinterpret_cast<gvec2 *>(out)) + pty * g.opo + (int64_t)27 * g.ostride + lidx;
#pragma unroll
      for (int i = 0; i < 9; i++) q[(int64_t)i * g.ostride] = p[(int64_t)i * g.istride];
    }
  }
}

// ---- copies: the whole extended field (nSteps = 0), and the border refresh ------------------------------------------------------------
struct CopyGeom {
  int volExCB;
  int istride, ostride;
  int64_t ipo, opo;
};

// every extended site of `in` to `out`, plane by plane (blockIdx.y = parity * 36 + plane); pads are not touched
template <typename FG> __global__ __launch_bounds__(kCopyThreads) void copy_extended_kernel(FG *out, const FG *in, CopyGeom g) {
  typedef FG gvec2 __attribute__((ext_vector_type(2)));
  const int x = blockIdx.x * kCopyThreads + threadIdx.x;
  if (x >= g.volExCB) return;
  const int pty = blockIdx.y / 36, plane = blockIdx.y - 36 * pty;
  const MUGIQ_GLOBAL gvec2 *p = as_global(reinterpret_cast<const gvec2 *>(in)) + pty * g.ipo + (int64_t)plane * g.istride;
  MUGIQ_GLOBAL gvec2 *q = as_global(reinterpret_cast<gvec2 *>(out)) + pty * g.opo + (int64_t)plane * g.ostride;
  q[x] = p[x];
}

struct SlabGeom {
  int XE[4];
  int d, R, X;  // the dimension, its border depth and its interior extent
  int nSites;   // R * the extended extents of the other three dimensions
  int stride;
  int64_t po;
};

// slab site s (x fastest, then y, z, t, the extent along d being R) with its layers starting at lo -> extended coordinates
__device__ inline void slab_coords(int c[4], int s, const SlabGeom &g, int lo) {
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int n = e == g.d ? g.R : g.XE[e];
    const int q = s / n;
    c[e] = s - q * n + (e == g.d ? lo : 0);
    s = q;
  }
}
__device__ inline int64_t slab_element(const int c[4], const SlabGeom &g, int plane) {
  const int pty = (c[0] + c[1] + c[2] + c[3]) & 1;
  return pty * g.po + (int64_t)plane * g.stride + (lex_index(c, g.XE) >> 1);
}

// MODE 0: wrap inside the domain (both borders from the interior layers at the other end);  1: pack the first R and the last R
// interior layers into buf[2][36][nSites];  2: unpack buf (received: [0] for the HIGH border, [1] for the LOW border).
// blockIdx.y = side * 36 + plane
template <typename FG, int MODE> __global__ __launch_bounds__(kCopyThreads) void border_kernel(FG *U, FG *buf, SlabGeom g) {
  typedef FG gvec2 __attribute__((ext_vector_type(2)));
  const int s = blockIdx.x * kCopyThreads + threadIdx.x;
  if (s >= g.nSites) return;
  const int side = blockIdx.y / 36, plane = blockIdx.y - 36 * side;
  MUGIQ_GLOBAL gvec2 *u = as_global(reinterpret_cast<gvec2 *>(U));
  const int64_t slot = ((int64_t)side * 36 + plane) * g.nSites + s;
  int c[4];
  if constexpr (MODE == 0) {
    // side 0: the HIGH border [R + X, R + X + R) from the layers [R, 2R);  side 1: the LOW border [0, R) from [X, X + R)
    slab_coords(c, s, g, side == 0 ? g.R : g.X);
    const int64_t from = slab_element(c, g, plane);
    slab_coords(c, s, g, side == 0 ? g.R + g.X : 0);
    u[slab_element(c, g, plane)] = u[from];
  } else if constexpr (MODE == 1) {
    slab_coords(c, s, g, side == 0 ? g.R : g.X);  // [0]: the first R interior layers, [1]: the last R
    as_global(reinterpret_cast<gvec2 *>(buf))[slot] = u[slab_element(c, g, plane)];
  } else {
    slab_coords(c, s, g, side == 0 ? g.R + g.X : 0);
    u[slab_element(c, g, plane)] = as_global(reinterpret_cast<gvec2 *>(buf))[slot];
  }
}

// ---- plaquette ---------------------------------------------------------------------------------------------------------------------------
// Re tr [ U_m(x) U_n(x+m) U_m^dag(x+n) U_n^dag(x) ] = Re sum_ij (U_m(x) U_n(x+m))_ij conj((U_n(x) U_m(x+n))_ij)
template <typename FG, int M, int N> __device__ inline double plaquette_plane(const FG *U, const SmearGeom &g, const int c2[4], int pty) {
  C64 a[9], b[9], w[9], w2[9];
  load_link<FG, M, N>(a, U, g, c2, pty, M, 0, 0);
  load_link<FG, M, N>(b, U, g, c2, pty, N, 1, 0);
  mul_nn(w, a, b);
  load_link<FG, M, N>(a, U, g, c2, pty, N, 0, 0);
  load_link<FG, M, N>(b, U, g, c2, pty, M, 0, 1);
  mul_nn(w2, a, b);
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    t = fma(w[i].re, w2[i].re, t);
    t = fma(w[i].im, w2[i].im, t);
  }
  return t;
}

// partial[group][2] = the workgroup's sums of Re tr P over the spatial and over the temporal planes, in a fixed order (tree over LDS)
template <typename FG> __global__ __launch_bounds__(kPlaqThreads) void plaquette_kernel(const FG *U, SmearGeom g, double *partial) {
  double acc[2] = {0.0, 0.0};
  for (int site = blockIdx.x * kPlaqThreads + threadIdx.x; site < 2 * g.volumeCB; site += gridDim.x * kPlaqThreads) {
    const int pty = site >= g.volumeCB ? 1 : 0;
    const int x_cb = site - pty * g.volumeCB;
    int coord[4], c2[4];
    get_coords(coord, x_cb, g.X, pty);
#pragma unroll
    for (int i = 0; i < 4; i++) c2[i] = coord[i] + g.brd[i];
    acc[0] += plaquette_plane<FG, 0, 1>(U, g, c2, pty);
    __builtin_amdgcn_sched_barrier(0);
    acc[0] += plaquette_plane<FG, 0, 2>(U, g, c2, pty);
    __builtin_amdgcn_sched_barrier(0);
    acc[0] += plaquette_plane<FG, 1, 2>(U, g, c2, pty);
    __builtin_amdgcn_sched_barrier(0);
    acc[1] += plaquette_plane<FG, 0, 3>(U, g, c2, pty);
    __builtin_amdgcn_sched_barrier(0);
    acc[1] += plaquette_plane<FG, 1, 3>(U, g, c2, pty);
    __builtin_amdgcn_sched_barrier(0);
    acc[1] += plaquette_plane<FG, 2, 3>(U, g, c2, pty);
  }
  __shared__ double sh[2][kPlaqThreads];
  const int t = threadIdx.x;
  sh[0][t] = acc[0];
  sh[1][t] = acc[1];
  __syncthreads();
  for (int s = kPlaqThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      sh[0][t] += sh[0][t + s];
      sh[1][t] += sh[1][t + s];
    }
    __syncthreads();
  }
  if (t < 2) partial[(size_t)blockIdx.x * 2 + t] = sh[t][0];
}

// out[k] = sum over the groups, in group order
__global__ void plaquette_final_sum_kernel(const double *partial, int nGroups, double *out) {
  const int k = threadIdx.x;
  if (k >= 2) return;
  double s = 0.0;
  for (int c = 0; c < nGroups; c++) s += partial[(size_t)c * 2 + k];
  out[k] = s;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// the descriptor of a field an entry point reads or writes; *volExCB: its extended checkerboard volume
int check_field(const MugiqHipGaugeField *U, const char *name, int *volExCB, const char *who) {
  MUGIQ_REQUIRE(U != nullptr && U->data != nullptr, "%s: gauge field %s is NULL", who, name);
  MUGIQ_REQUIRE(U->precision == 4 || U->precision == 8, "%s: precision %d of %s must be 4 or 8", who, U->precision, name);
  long long volEx = 1;
  int sumR = 0;
  for (int d = 0; d < 4; d++) {
    MUGIQ_REQUIRE(U->X[d] > 0 && (U->X[d] & 1) == 0, "%s: X[%d] = %d of %s must be positive and even", who, d, U->X[d], name);
    MUGIQ_REQUIRE(U->R[d] >= 0 && U->R[d] <= U->X[d], "%s: R[%d] = %d of %s must be within [0, X[%d] = %d]", who, d, U->R[d], name, d, U->X[d]);
    volEx *= U->X[d] + 2 * U->R[d];
    sumR += U->R[d];
  }
  MUGIQ_REQUIRE((sumR & 1) == 0, "%s: the sum of the borders R of %s must be even", who, name);
  MUGIQ_REQUIRE(volEx / 2 < (1LL << 30), "%s: extended volume of %s overflows int", who, name);
  MUGIQ_REQUIRE(U->stride >= volEx / 2, "%s: stride %d of %s < extended volumeCB %lld", who, U->stride, name, volEx / 2);
  MUGIQ_REQUIRE(U->parity_offset >= (int64_t)36 * U->stride, "%s: parity_offset %lld of %s < 36*stride", who, (long long)U->parity_offset, name);
  *volExCB = (int)(volEx / 2);
  return MUGIQ_HIP_SUCCESS;
}

// comm -> part[4]; a partitioned dimension needs a border and the halo callback
int check_partitioning(const MugiqHipGaugeField *U, const MugiqHipComm *comm, int part[4], bool needSums, const char *who) {
  if (int st = check_comm(comm, part, needSums, who)) return st;
  for (int d = 0; d < 4; d++)
    MUGIQ_REQUIRE(!part[d] || U->R[d] >= 1, "%s: dimension %d is partitioned but the gauge field has no border along it (R = 0)", who, d);
  return MUGIQ_HIP_SUCCESS;
}

SmearGeom smear_geom(const MugiqHipGaugeField &in, const MugiqHipGaugeField &out) {
  SmearGeom g;
  long long vol = 1;
  for (int d = 0; d < 4; d++) {
    g.X[d] = in.X[d];
    g.brd[d] = in.R[d];
    g.XE[d] = in.X[d] + 2 * in.R[d];
    vol *= in.X[d];
  }
  g.volumeCB = (int)(vol / 2);
  g.istride = in.stride;
  g.ipo = in.parity_offset;
  g.ostride = out.stride;
  g.opo = out.parity_offset;
  return g;
}

size_t slab_bytes(const MugiqHipGaugeField &U, int d) {
  size_t n = (size_t)U.R[d];
  for (int e = 0; e < 4; e++)
    if (e != d) n *= (size_t)(U.X[e] + 2 * U.R[e]);
  return n * 2 * 36 * 2 * (size_t)U.precision;  // both ends, 36 planes, complex
}

// the R-deep borders of U from its interior; send / recv: device buffers of the largest partitioned slab (may be NULL if there is none)
template <typename FG> int exchange_borders(const MugiqHipGaugeField &U, const MugiqHipComm *comm, const int part[4], void *send, void *recv,
                                            hipStream_t s, const char *who) {
  for (int d = 0; d < 4; d++) {
    if (U.R[d] == 0) continue;
    SlabGeom g;
    g.nSites = U.R[d];
    for (int e = 0; e < 4; e++) {
      g.XE[e] = U.X[e] + 2 * U.R[e];
      if (e != d) g.nSites *= g.XE[e];
    }
    g.d = d;
    g.R = U.R[d];
    g.X = U.X[d];
    g.stride = U.stride;
    g.po = U.parity_offset;
    const dim3 grid((g.nSites + kCopyThreads - 1) / kCopyThreads, 72), block(kCopyThreads);
    FG *u = static_cast<FG *>(U.data);
    if (!part[d]) {
      hipLaunchKernelGGL((border_kernel<FG, 0>), grid, block, 0, s, u, static_cast<FG *>(nullptr), g);
      MUGIQ_CHECK_HIP(hipGetLastError());
      continue;
    }
    hipLaunchKernelGGL((border_kernel<FG, 1>), grid, block, 0, s, u, static_cast<FG *>(send), g);
    MUGIQ_CHECK_HIP(hipGetLastError());
    // the first R interior layers go backward and fill that neighbour's HIGH border: what arrives from the forward neighbour fills mine
    const size_t half = slab_bytes(U, d) / 2;
    for (int pass = 0; pass < 2; pass++) {
      const int st = comm->sendrecv(comm->ctx, static_cast<char *>(send) + pass * half, static_cast<char *>(recv) + pass * half, half, d,
                                    pass == 0 ? -1 : +1, s);
      if (st) return set_error(MUGIQ_HIP_ERROR_HIP, "%s: halo sendrecv callback failed with status %d", who, st);
    }
    hipLaunchKernelGGL((border_kernel<FG, 2>), grid, block, 0, s, u, static_cast<FG *>(recv), g);
    MUGIQ_CHECK_HIP(hipGetLastError());
  }
  return MUGIQ_HIP_SUCCESS;
}

// device buffers for the partitioned slabs of U, released by the destructor (after the stream has drained)
struct HaloBuffers {
  void *send = nullptr, *recv = nullptr;
  hipStream_t stream = nullptr;
  int alloc(const MugiqHipGaugeField &U, const int part[4], hipStream_t s) {
    stream = s;
    size_t bytes = 0;
    for (int d = 0; d < 4; d++)
      if (part[d] && U.R[d] > 0) bytes = std::max(bytes, slab_bytes(U, d));
    if (bytes == 0) return MUGIQ_HIP_SUCCESS;
    MUGIQ_CHECK_HIP(hipMalloc(&send, bytes));
    MUGIQ_CHECK_HIP(hipMalloc(&recv, bytes));
    return MUGIQ_HIP_SUCCESS;
  }
  ~HaloBuffers() {
    if (send || recv) (void)hipStreamSynchronize(stream);
    if (send) (void)hipFree(send);
    if (recv) (void)hipFree(recv);
  }
};

struct TempField {
  void *data = nullptr;
  hipStream_t stream = nullptr;
  ~TempField() {
    if (data) {
      (void)hipStreamSynchronize(stream);
      (void)hipFree(data);
    }
  }
};

template <typename FG>
int stout_steps(const MugiqHipGaugeField &out, const MugiqHipGaugeField &in, int volExCB, double rho, int nSteps, int smearDims,
                const MugiqHipComm *comm, const int part[4], hipStream_t s, const char *who) {
  HaloBuffers halo;
  if (int st = halo.alloc(out, part, s)) return st;
  if (nSteps == 0) {
    const CopyGeom c{volExCB, in.stride, out.stride, in.parity_offset, out.parity_offset};
    hipLaunchKernelGGL((copy_extended_kernel<FG>), dim3((volExCB + kCopyThreads - 1) / kCopyThreads, 72), dim3(kCopyThreads), 0, s,
                       static_cast<FG *>(out.data), static_cast<const FG *>(in.data), c);
    MUGIQ_CHECK_HIP(hipGetLastError());
    return exchange_borders<FG>(out, comm, part, halo.send, halo.recv, s, who);
  }
  // ping-pong between `out` and one temporary field of its geometry (pad 0), so that the last step lands in `out`
  TempField tmp;
  MugiqHipGaugeField T = out;
  if (nSteps >= 2) {
    T.stride = volExCB;
    T.parity_offset = (int64_t)36 * volExCB;
    tmp.stream = s;
    MUGIQ_CHECK_HIP(hipMalloc(&tmp.data, (size_t)2 * T.parity_offset * 2 * sizeof(FG)));
    T.data = tmp.data;
  }
  const MugiqHipGaugeField *src = &in;
  for (int k = 0; k < nSteps; k++) {
    const MugiqHipGaugeField *dst = ((nSteps - 1 - k) & 1) ? &T : &out;
    const SmearGeom g = smear_geom(*src, *dst);
    const dim3 grid((2 * g.volumeCB + kStoutThreads - 1) / kStoutThreads, 4), block(kStoutThreads);
    if (smearDims == 3)
      hipLaunchKernelGGL((stout_kernel<FG, 3>), grid, block, 0, s, static_cast<FG *>(dst->data), static_cast<const FG *>(src->data), g, rho);
    else
      hipLaunchKernelGGL((stout_kernel<FG, 4>), grid, block, 0, s, static_cast<FG *>(dst->data), static_cast<const FG *>(src->data), g, rho);
    MUGIQ_CHECK_HIP(hipGetLastError());
    if (int st = exchange_borders<FG>(*dst, comm, part, halo.send, halo.recv, s, who)) return st;
    src = dst;
  }
  return MUGIQ_HIP_SUCCESS;
}

template <typename FG> int plaquette_sums(const MugiqHipGaugeField &U, double sums[2], hipStream_t s) {
  const SmearGeom g = smear_geom(U, U);
  const int nGroups = std::min(kPlaqMaxGroups, (2 * g.volumeCB + kPlaqThreads - 1) / kPlaqThreads);
  void *ws = nullptr;
  if (int st = stream_workspace(&ws, sizeof(double) * 2 * ((size_t)nGroups + 1), s)) return st;
  double *partial = static_cast<double *>(ws), *res = partial + (size_t)2 * nGroups;
  hipLaunchKernelGGL((plaquette_kernel<FG>), dim3(nGroups), dim3(kPlaqThreads), 0, s, static_cast<const FG *>(U.data), g, partial);
  MUGIQ_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(plaquette_final_sum_kernel, dim3(1), dim3(64), 0, s, partial, nGroups, res);
  MUGIQ_CHECK_HIP(hipGetLastError());
  MUGIQ_CHECK_HIP(hipMemcpyAsync(sums, res, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
  MUGIQ_CHECK_HIP(hipStreamSynchronize(s));
  return MUGIQ_HIP_SUCCESS;
}

// [first, last) byte range the kernels may touch
void gauge_span(const MugiqHipGaugeField &U, uintptr_t *a, uintptr_t *b) {
  *a = reinterpret_cast<uintptr_t>(U.data);
  *b = *a + (uintptr_t)(U.parity_offset + (int64_t)36 * U.stride) * 2 * U.precision;
}

}  // namespace
}  // namespace mugiq

using namespace mugiq;

extern "C" {

int mugiq_hip_exchange_extended_gauge(const MugiqHipGaugeField *gauge, const MugiqHipComm *comm, void *stream) {
  const char *who = "exchangeExtendedGauge";
  int st, part[4], volExCB;
  if ((st = check_field(gauge, "gauge", &volExCB, who))) return st;
  if ((st = check_partitioning(gauge, comm, part, false, who))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  HaloBuffers halo;
  if ((st = halo.alloc(*gauge, part, s))) return st;
  if (gauge->precision == 8) return exchange_borders<double>(*gauge, comm, part, halo.send, halo.recv, s, who);
  return exchange_borders<float>(*gauge, comm, part, halo.send, halo.recv, s, who);
}

int mugiq_hip_stout_smear(const MugiqHipGaugeField *out, const MugiqHipGaugeField *in, double rho, int nSteps, int smearDims,
                          const MugiqHipComm *comm, void *stream) {
  const char *who = "stoutSmear";
  int st, part[4], volExCB, volExCBin;
  if ((st = check_field(out, "out", &volExCB, who))) return st;
  if ((st = check_field(in, "in", &volExCBin, who))) return st;
  MUGIQ_REQUIRE(in->precision == out->precision, "%s: precision %d of in differs from %d of out", who, in->precision, out->precision);
  for (int d = 0; d < 4; d++)
    MUGIQ_REQUIRE(in->X[d] == out->X[d] && in->R[d] == out->R[d], "%s: X[%d] = %d, R[%d] = %d of in differ from %d, %d of out", who, d, in->X[d], d,
                  in->R[d], out->X[d], out->R[d]);
  uintptr_t a0, a1, b0, b1;
  gauge_span(*in, &a0, &a1);
  gauge_span(*out, &b0, &b1);
  MUGIQ_REQUIRE(a1 <= b0 || b1 <= a0, "%s: the buffers of in and out overlap", who);
  MUGIQ_REQUIRE(nSteps >= 0, "%s: nSteps = %d is negative", who, nSteps);
  MUGIQ_REQUIRE(smearDims == 3 || smearDims == 4, "%s: smearDims = %d must be 3 or 4", who, smearDims);
  MUGIQ_REQUIRE(std::isfinite(rho), "%s: rho is not finite", who);
  if ((st = check_partitioning(out, comm, part, false, who))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  if (out->precision == 8) return stout_steps<double>(*out, *in, volExCB, rho, nSteps, smearDims, comm, part, s, who);
  return stout_steps<float>(*out, *in, volExCB, rho, nSteps, smearDims, comm, part, s, who);
}

int mugiq_hip_plaquette(const MugiqHipGaugeField *gauge, double plaq_h[3], const MugiqHipComm *comm, void *stream) {
  const char *who = "plaquette";
  int st, part[4], volExCB;
  if ((st = check_field(gauge, "gauge", &volExCB, who))) return st;
  MUGIQ_REQUIRE(plaq_h != nullptr, "%s: plaq_h is NULL", who);
  if ((st = check_partitioning(gauge, comm, part, true, who))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  double sums[2];
  if ((st = gauge->precision == 8 ? plaquette_sums<double>(*gauge, sums, s) : plaquette_sums<float>(*gauge, sums, s))) return st;
  double ranks = 1.0;
  if (comm && comm->size > 1) {
    std::vector<double> v(sums, sums + 2);
    if ((st = sum_over_ranks(comm, v))) return st;
    sums[0] = v[0];
    sums[1] = v[1];
    ranks = (double)comm->size;
  }
  // Re tr / 3, three planes each, every site of every rank
  const double norm = 9.0 * ranks * (double)gauge->X[0] * (double)gauge->X[1] * (double)gauge->X[2] * (double)gauge->X[3];
  plaq_h[1] = sums[0] / norm;
  plaq_h[2] = sums[1] / norm;
  plaq_h[0] = 0.5 * (plaq_h[1] + plaq_h[2]);
  return MUGIQ_HIP_SUCCESS;
}

}  // extern "C"
