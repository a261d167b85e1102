// Fused displaced contraction in an axial gauge on the fp64 matrix pipe (fourth generation).  Column tiles for mu = y, z, t, whole x rows
// for mu = x; ascending lengths up to 8 per entry; eigenvectors fp64 FLOAT2 (every tile geometry, and the face layers of posted halos
// written on the way) or fp64 FLOAT4 / fp32 FLOAT2 / fp32 FLOAT4 (converted on their way into LDS; 16-line tiles); slots fp64 or fp32.
//
// (1) The gauge.  Along every line of direction mu fix g(j + 1) = g(j) U_mu(x_j), g(0) = 1 (continued past both ends of
// the local line with the path-link products the driver has anyway: g(J + l) = g(J - 1) W_{l+1}(x_{J-1}), g(-l) = W^-_l(x_0)).
// Then g(x) U_mu(x) g(x + mu)^dag = 1, i.e. W_k(x) psi(x + k mu) = g(x)^dag [g psi](x + k mu), and because the colour trace
// does not see a unitary rotation of both factors
//        sum_c conj(v(x)[be][c]) (W_k(x) v(x + k mu))[al][c]  =  sum_c conj(v'(x)[be][c]) v'(x + k mu)[al][c],   v' = g v.
// The tile applies g ONCE per staged position and eigenvector (9 complex FMAs per spin) on the way into LDS, instead of W_k
// once per slot: 36 (4 + Kmax)/4 + 48 Kmax complex FMAs per site where csrc/fused_tile.hip spends 84 Kmax (Kmax = 3:
// 207 against 252), and no link field is read by the contraction any more.
//
// (2) The matrix pipe.  What is left per site, slot and eigenvector is a 4 x 3 times 3 x 4 complex product -- one block of
// v_mfma_f64_4x4x4_4b_f64 (four independent 4x4x4 products per instruction, ONE LATTICE SITE PER BLOCK):
//     lane maps (tools/probes/mfma_4x4x4_layout.hip, one-hot operands):
//       A[b][i][k] in lane 16 k + 4 b + i,   B[b][k][j] in lane 16 k + 4 b + j,   D[b][i][j] in lane 16 i + 4 b + j
//     accR[be][al] += VR[be][c] PR[c][al] + VI[be][c] PI[c][al]          V = v'(x) / sigma_n, P = v'(x + k mu)
//     accI[be][al] += VR[be][c] PI[c][al] - VI[be][c] PR[c][al]          (colour index c padded 3 -> 4 with V = 0)
// Four products of 128 flops do the 384 flops of the outer product (75 %); V and P come from LDS with ONE ds_read_b128 per
// lane and 4-site group each (V is shared by the slots) and ARE the operands as they stand; the 4x4 colour-traced spin
// matrices accumulate in the D registers (2 x 2 VGPRs per group and slot).
//
// Tile and pipeline as csrc/fused_tile.hip: a workgroup owns 32 lines along mu x 4 consecutive positions and needs 4 + Kmax
// staged positions; thread (position, spin, line) loads its three colours two eigenvectors ahead into registers, rotates
// them with its g (in registers for the whole kernel) and commits v' to the other LDS buffer while the products of the
// current eigenvector run; one LDS-only barrier per eigenvector.
// LDS image: chunk (position pair, component) = [position & 1][32 lines] complex = 1 KiB, chunks 64 bytes apart in bank
// phase (stride 1088 B): an operand read -- lanes (colour, site, spin) -> component 3 spin + colour -- touches every bank
// once.  Measurements, and the form with W_k applied on the matrix pipe that this one replaces: profiles/r04_mfma_tile.txt.
#include "fused_mfma_kernel.h"

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

namespace mugiq {

// ---- the axial gauge of one (direction, sign) from the path-link fields E_k = W_k (FLOAT2, pad 0; component 3 j + i of
// E_k(x) is W_k(x)[i][j]): one thread per line, sequential along the line
// ---- unitarity of the axial gauge.  W_k(x) v(x + k mu) = g(x)^dag [g v](x + k mu) needs g^dag g = 1; with links that are not unitary
// (anisotropy-rescaled, smeared and not re-projected, fp32 links in fp64 storage) the tile's error is (g(x)^dag g(x) - 1) W_k(x).
// mt_deviation: max_ab |(g^dag g - 1)_ab|.  Maxima go into a device word as the bits of a non-negative double (they order like the
// values); a NaN stays NaN, and no threshold passes it.
__device__ inline double mt_deviation(const Cplx<double> g[9]) {
  double d = 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) {
      Cplx<double> s{a == b ? -1.0 : 0.0, 0.0};
#pragma unroll
      for (int m = 0; m < 3; m++) cmadd_conj(s, g[m * 3 + a], g[m * 3 + b]);
      const double e = sqrt(s.re * s.re + s.im * s.im);
      d = (e > d || e != e) ? e : d;
    }
  return d;
}
__device__ inline void mt_worse(double &worst, double d) { worst = (d > worst || d != d) ? d : worst; }
__device__ inline void mt_report(unsigned long long *out, double worst) { atomicMax(out, (unsigned long long)__double_as_longlong(worst)); }

template <typename F> struct AxialArgs {
  Cplx<double> *G;
  unsigned long long *dev;  // != NULL: also the largest deviation of the gauge built (mt_deviation)
  const Cplx<F> *E[kMT_MaxLength];  // E_1 .. E_kmax (storage precision; the gauge itself is kept in double)
  int kmax, sign, J, strideMu, H, numCols, volumeCB;
  int rowMode, X1, X2;  // mu = x: line = x row `cid`, site j <-> (parity p0 ^ (j & 1), entry cid J/2 + j/2); G is [9][row][position]
};
template <typename F> __device__ inline void mt_load_w(Cplx<double> w[9], const Cplx<F> *E, int par, int x_cb, int volumeCB) {
  const Cplx<F> *e = E + (int64_t)par * 12 * volumeCB + x_cb;
#pragma unroll
  for (int j = 0; j < 3; j++)
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const Cplx<F> u = e[(int64_t)(j * 3 + i) * volumeCB];
      w[i * 3 + j] = Cplx<double>{(double)u.re, (double)u.im};
    }
}
// r = x y (DAG: x y^dag)
template <bool DAG> __device__ inline void mt_mul3(Cplx<double> r[9], const Cplx<double> x[9], const Cplx<double> y[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      Cplx<double> s{0.0, 0.0};
#pragma unroll
      for (int m = 0; m < 3; m++) {
        if (DAG) cmadd(s, x[i * 3 + m], Cplx<double>{y[j * 3 + m].re, -y[j * 3 + m].im});
        else cmadd(s, x[i * 3 + m], y[m * 3 + j]);
      }
      r[i * 3 + j] = s;
    }
}
template <typename F> __global__ __launch_bounds__(64) void axial_gauge_kernel(AxialArgs<F> a) {
  const int cid = blockIdx.x * 64 + threadIdx.x;
  if (cid >= a.numCols) return;
  int p0, base;
  if (a.rowMode) {
    const int zt = cid / a.X1;
    p0 = (cid % a.X1 + zt % a.X2 + zt / a.X2) & 1;
    base = cid * (a.J >> 1);
  } else {
    mt_line(cid, a.H, a.strideMu, a.J, p0, base);
  }
  const int Jext = a.J + a.kmax;
  auto store = [&](int jext, const Cplx<double> g[9]) {
#pragma unroll
    for (int c = 0; c < 9; c++) a.G[a.rowMode ? ((int64_t)c * a.numCols + cid) * Jext + jext : ((int64_t)c * Jext + jext) * a.numCols + cid] = g[c];
  };
  auto site_xcb = [&](int j) { return a.rowMode ? base + (j >> 1) : base + j * a.strideMu; };
  double worst = 0.0;
  auto store_checked = [&](int jext, const Cplx<double> g[9]) {
    store(jext, g);
    if (a.dev) mt_worse(worst, mt_deviation(g));
  };
  Cplx<double> g[9], w[9], t[9];
#pragma unroll
  for (int c = 0; c < 9; c++) g[c] = Cplx<double>{c % 4 == 0 ? 1.0 : 0.0, 0.0};
  const int off = a.sign == MUGIQ_HIP_DISP_SIGN_PLUS ? 0 : a.kmax;
  if (a.sign == MUGIQ_HIP_DISP_SIGN_MINUS) {  // g(-l) = W^-_l(x_0)
    for (int l = 1; l <= a.kmax; l++) {
      mt_load_w(w, a.E[l - 1], p0, site_xcb(0), a.volumeCB);
      store_checked(a.kmax - l, w);
    }
  }
  for (int j = 0; j < a.J; j++) {
    const int par = p0 ^ (j & 1), x_cb = site_xcb(j);
    if (a.sign == MUGIQ_HIP_DISP_SIGN_MINUS && j > 0) {  // g(j) = g(j - 1) W^-_1(x_j)^dag      (W^-_1(x) = U(x - mu)^dag)
      mt_load_w(w, a.E[0], par, x_cb, a.volumeCB);
      mt_mul3<true>(t, g, w);
#pragma unroll
      for (int c = 0; c < 9; c++) g[c] = t[c];
    }
    store_checked(j + off, g);
    if (a.sign == MUGIQ_HIP_DISP_SIGN_PLUS) {
      if (j == a.J - 1) {  // g(J + l) = g(J - 1) W_{l+1}(x_{J-1})
        for (int l = 0; l < a.kmax; l++) {
          mt_load_w(w, a.E[l], par, x_cb, a.volumeCB);
          mt_mul3<false>(t, g, w);
          store_checked(a.J + l, t);
        }
      } else {  // g(j + 1) = g(j) W_1(x_j)
        mt_load_w(w, a.E[0], par, x_cb, a.volumeCB);
        mt_mul3<false>(t, g, w);
#pragma unroll
        for (int c = 0; c < 9; c++) g[c] = t[c];
      }
    }
  }
  if (a.dev) mt_report(a.dev, worst);
}

// ---- the same gauge straight from the gauge field, for a direction that is NOT partitioned (the local line is the global, periodic
// one): W_1(x) = U_mu(x), so g(j + 1) = g(j) U_mu(x_j) for either sign, continued with the links of the wrapped sites --
// g(J + l) = g(J + l - 1) U(x_{(J + l - 1) mod J}), g(-l) = g(-l + 1) U(x_{J - l})^dag -- and no path-link field has to be built at all
// (the driver's chain of `stop` covariant displacements of the identity: 0.4 ms and a GB of scratch per entry at configs[2]).
template <typename F> struct AxialLinkArgs {
  Cplx<double> *G;
  const Cplx<F> *U;   // extended gauge field: parity * Upo + (dir * 9 + row * 3 + col) * Ustride + x_cb on the extended lattice
  int64_t Upo;
  int Ustride;
  int X[4], R[4];
  int dir, kmax, sign, J, strideMu, H, numCols;
  int rowMode;
};
template <typename F> __global__ __launch_bounds__(64) void axial_gauge_from_links_kernel(AxialLinkArgs<F> a) {
  const int cid = blockIdx.x * 64 + threadIdx.x;
  if (cid >= a.numCols) return;
  int p0, base;
  if (a.rowMode) {
    const int zt = cid / a.X[1];
    p0 = (cid % a.X[1] + zt % a.X[2] + zt / a.X[2]) & 1;
    base = cid * (a.J >> 1);
  } else {
    mt_line(cid, a.H, a.strideMu, a.J, p0, base);
  }
  int c0[4], XE[4];
  get_coords(c0, base, a.X, p0);  // the j = 0 site of the line (row mode: x = 0 or 1 -- only the other three coordinates are used)
#pragma unroll
  for (int d = 0; d < 4; d++) XE[d] = a.X[d] + 2 * a.R[d];
  // U_mu at position j of the line; j < 0 or j >= J: the wrapped site of a periodic line, or -- along a partitioned direction -- the
  // neighbour's link in the border of the extended field (-R <= j < J + R)
  auto load_u = [&](Cplx<double> u[9], int j) {
    const int jj = a.R[a.dir] > 0 ? j : ((j % a.J) + a.J) % a.J;
    int c[4];
#pragma unroll
    for (int d = 0; d < 4; d++) c[d] = (d == a.dir ? jj : c0[d]) + a.R[d];
    const int par = p0 ^ (j & 1);  // (borders are even in sum: the extended parity is the interior one)
    const Cplx<F> *q = a.U + (int64_t)par * a.Upo + (int64_t)(a.dir * 9) * a.Ustride + (lex_index(c, XE) >> 1);
#pragma unroll
    for (int e = 0; e < 9; e++) {
      const Cplx<F> v = q[(int64_t)e * a.Ustride];
      u[e] = Cplx<double>{(double)v.re, (double)v.im};
    }
  };
  const int Jext = a.J + a.kmax;
  auto store = [&](int jext, const Cplx<double> g[9]) {
#pragma unroll
    for (int c = 0; c < 9; c++) a.G[a.rowMode ? ((int64_t)c * a.numCols + cid) * Jext + jext : ((int64_t)c * Jext + jext) * a.numCols + cid] = g[c];
  };
  Cplx<double> g[9], w[9], t[9];
#pragma unroll
  for (int c = 0; c < 9; c++) g[c] = Cplx<double>{c % 4 == 0 ? 1.0 : 0.0, 0.0};
  const int off = a.sign == MUGIQ_HIP_DISP_SIGN_PLUS ? 0 : a.kmax;
  if (a.sign == MUGIQ_HIP_DISP_SIGN_MINUS) {  // g(-l) = g(-l + 1) U(x_{J - l})^dag
    for (int l = 1; l <= a.kmax; l++) {
      load_u(w, -l);
      mt_mul3<true>(t, g, w);
#pragma unroll
      for (int c = 0; c < 9; c++) g[c] = t[c];
      store(a.kmax - l, g);
    }
#pragma unroll
    for (int c = 0; c < 9; c++) g[c] = Cplx<double>{c % 4 == 0 ? 1.0 : 0.0, 0.0};
  }
  const int last = a.sign == MUGIQ_HIP_DISP_SIGN_PLUS ? a.J + a.kmax : a.J;
  for (int j = 0; j < last; j++) {
    store(j + off, g);
    if (j + 1 < last) {
      load_u(w, j);
      mt_mul3<false>(t, g, w);
#pragma unroll
      for (int c = 0; c < 9; c++) g[c] = t[c];
    }
  }
}

static int launch_mfma_tile(const MTileArgs &a, int precision, int order, int dir, int sign, int ns, const MfmaLaunch &g, hipStream_t stream) {
  if (a.VL) {  // two-sided
    if (precision == 8 && order == 2) return launch_mfma_tile_two_d2(a, dir, sign, ns, g, stream);
    if (precision == 8) return launch_mfma_tile_two_d4(a, dir, sign, ns, g, stream);
    if (order == 2) return launch_mfma_tile_two_f2(a, dir, sign, ns, g, stream);
    return launch_mfma_tile_two_f4(a, dir, sign, ns, g, stream);
  }
  if (precision == 8 && order == 2) return launch_mfma_tile_t<double, 2, true>(a, dir, sign, ns, g, stream);
  if (precision == 8) return launch_mfma_tile_d4(a, dir, sign, ns, g, stream);
  if (order == 2) return launch_mfma_tile_f2(a, dir, sign, ns, g, stream);
  return launch_mfma_tile_f4(a, dir, sign, ns, g, stream);
}

template <typename F>
static int build_axial_gauge_t(void *G_d, const MugiqHipSpinorField &ev, const void *const *E_d, int kmax, int dir, int sign, hipStream_t stream,
                               unsigned long long *dev_d) {
  AxialArgs<F> g;
  g.G = static_cast<Cplx<double> *>(G_d);
  g.dev = dev_d;
  for (int l = 0; l < kMT_MaxLength; l++) g.E[l] = static_cast<const Cplx<F> *>(E_d[l < kmax ? l : 0]);
  const LineGeometry lines = line_geometry(ev, dir);
  g.kmax = kmax;
  g.sign = sign;
  g.J = ev.X[dir];
  g.strideMu = lines.strideMu;
  g.H = lines.H;
  g.numCols = lines.numCols;
  g.volumeCB = ev.volumeCB;
  g.rowMode = dir == 0;
  g.X1 = ev.X[1];
  g.X2 = ev.X[2];
  hipLaunchKernelGGL(axial_gauge_kernel<F>, dim3((g.numCols + 63) / 64), dim3(64), 0, stream, g);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}
// (the path-link fields are FLOAT2, pad 0, in the eigenvectors' precision)
int build_axial_gauge(void *G_d, const MugiqHipSpinorField &ev, const void *const *E_d, int kmax, int dir, int sign, hipStream_t stream) {
  return ev.precision == 8 ? build_axial_gauge_t<double>(G_d, ev, E_d, kmax, dir, sign, stream, nullptr)
                           : build_axial_gauge_t<float>(G_d, ev, E_d, kmax, dir, sign, stream, nullptr);
}

double axial_gauge_tolerance(int precision) { return precision == 8 ? 1e-12 : 4e-6; }

static double deviation_from_bits(unsigned long long b) {
  double d;
  std::memcpy(&d, &b, sizeof d);
  return d;
}

// The free fused call: the gauge from the links of the call into the stream's workspace, and its largest deviation (host-blocking)
int build_axial_gauge_checked(void **G_out, double *deviation, const MugiqHipSpinorField &ev, const void *const *E_d, int kmax, int dir, int sign,
                              hipStream_t stream) {
  const size_t gb = axial_gauge_bytes_of(ev, dir, kmax);
  void *ws = nullptr;
  int st = stream_workspace(&ws, gb + 256, stream);
  if (st) return st;
  unsigned long long *dev_d = reinterpret_cast<unsigned long long *>(static_cast<char *>(ws) + gb);
  MUGIQ_CHECK_HIP(hipMemsetAsync(dev_d, 0, sizeof *dev_d, stream));
  st = ev.precision == 8 ? build_axial_gauge_t<double>(ws, ev, E_d, kmax, dir, sign, stream, dev_d)
                         : build_axial_gauge_t<float>(ws, ev, E_d, kmax, dir, sign, stream, dev_d);
  if (st) return st;
  unsigned long long bits = 0;
  MUGIQ_CHECK_HIP(hipMemcpyAsync(&bits, dev_d, sizeof bits, hipMemcpyDeviceToHost, stream));
  MUGIQ_CHECK_HIP(hipStreamSynchronize(stream));
  *G_out = ws;
  *deviation = deviation_from_bits(bits);
  return MUGIQ_HIP_SUCCESS;
}

// ---- the driver's pre-pass: D_mu = max over the lines of direction mu and the positions -reach .. J + reach - 1 of mt_deviation(g), with
// g(j + 1) = g(j) U_mu(x_j), g(0) = 1 (the recurrence of axial_gauge_from_links_kernel; a periodic line wraps, a partitioned one stops where
// the border of the extended field ends -- the neighbour's own pre-pass covers its links).  One thread per line.
template <typename F> struct DeviationArgs {
  const Cplx<F> *U;
  int64_t Upo;
  int Ustride;
  int X[4], R[4];
  int dir, fwd, bwd, periodic, numLines;
  unsigned long long *out;
};
template <typename F> __global__ __launch_bounds__(64) void axial_deviation_kernel(DeviationArgs<F> a) {
  const int cid = blockIdx.x * 64 + threadIdx.x;
  const bool line = cid < a.numLines;  // (every lane stays for the wave's reduction below)
  int c0[4], XE[4];
  for (int d = 0, r = cid; d < 4; d++) {
    XE[d] = a.X[d] + 2 * a.R[d];
    if (d == a.dir) {
      c0[d] = 0;
    } else {
      c0[d] = r % a.X[d];
      r /= a.X[d];
    }
  }
  const int J = a.X[a.dir];
  auto load_u = [&](Cplx<double> u[9], int j) {
    int c[4];
#pragma unroll
    for (int d = 0; d < 4; d++) c[d] = d == a.dir ? (a.periodic ? ((j % J) + J) % J : j) : c0[d];
    const int par = (c[0] + c[1] + c[2] + c[3]) & 1;  // (borders are even: the extended parity is the interior one)
#pragma unroll
    for (int d = 0; d < 4; d++) c[d] += a.R[d];
    const Cplx<F> *q = a.U + (int64_t)par * a.Upo + (int64_t)(a.dir * 9) * a.Ustride + (lex_index(c, XE) >> 1);
#pragma unroll
    for (int e = 0; e < 9; e++) {
      const Cplx<F> v = q[(int64_t)e * a.Ustride];
      u[e] = Cplx<double>{(double)v.re, (double)v.im};
    }
  };
  Cplx<double> g[9], u[9], t[9];
  double worst = 0.0;
  for (int pass = 0; pass < 2; pass++) {  // g(1) .. g(fwd), then g(-1) .. g(-bwd)
#pragma unroll
    for (int c = 0; c < 9; c++) g[c] = Cplx<double>{c % 4 == 0 ? 1.0 : 0.0, 0.0};
    const int n = !line ? 0 : pass == 0 ? a.fwd : a.bwd;
    for (int l = 0; l < n; l++) {
      load_u(u, pass == 0 ? l : -1 - l);
      if (pass == 0) mt_mul3<false>(t, g, u);
      else mt_mul3<true>(t, g, u);
#pragma unroll
      for (int c = 0; c < 9; c++) g[c] = t[c];
      mt_worse(worst, mt_deviation(g));
    }
  }
  for (int m = 32; m >= 1; m >>= 1) mt_worse(worst, __shfl_xor(worst, m, 64));  // one atomic per wave, not one per line
  if (threadIdx.x == 0) mt_report(a.out, worst);
}

template <typename F>
static int launch_axial_deviation(unsigned long long *out_d, const MugiqHipGaugeField &U, int dir, int reach, int partitioned, hipStream_t stream) {
  DeviationArgs<F> a;
  a.U = static_cast<const Cplx<F> *>(U.data);
  a.Upo = U.parity_offset;
  a.Ustride = U.stride;
  long long lines = 1;
  for (int d = 0; d < 4; d++) {
    a.X[d] = U.X[d];
    a.R[d] = U.R[d];
    if (d != dir) lines *= U.X[d];
  }
  a.dir = dir;
  a.periodic = !partitioned;
  const int J = U.X[dir];
  a.fwd = partitioned ? std::min(J + reach - 1, J + U.R[dir]) : J + reach - 1;  // (g(j + 1) needs the link at j)
  a.bwd = partitioned ? std::min(reach, U.R[dir]) : reach;
  a.numLines = (int)lines;
  a.out = out_d;
  hipLaunchKernelGGL(axial_deviation_kernel<F>, dim3((unsigned)((lines + 63) / 64)), dim3(64), 0, stream, a);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

int axial_line_deviation(double D[4], const MugiqHipGaugeField &U, const int reach[4], const int partitioned[4], hipStream_t stream) {
  void *ws = nullptr;
  int st = stream_workspace(&ws, 4 * sizeof(unsigned long long), stream);
  if (st) return st;
  unsigned long long *out_d = static_cast<unsigned long long *>(ws);
  MUGIQ_CHECK_HIP(hipMemsetAsync(out_d, 0, 4 * sizeof(unsigned long long), stream));
  for (int d = 0; d < 4; d++) {
    if (reach[d] <= 0) continue;
    const int r = std::min(reach[d], kMT_MaxLength);  // (longer entries never take the tile)
    st = U.precision == 8 ? launch_axial_deviation<double>(out_d + d, U, d, r, partitioned[d], stream)
                          : launch_axial_deviation<float>(out_d + d, U, d, r, partitioned[d], stream);
    if (st) return st;
  }
  unsigned long long bits[4] = {0, 0, 0, 0};
  MUGIQ_CHECK_HIP(hipMemcpyAsync(bits, out_d, sizeof bits, hipMemcpyDeviceToHost, stream));
  MUGIQ_CHECK_HIP(hipStreamSynchronize(stream));
  for (int d = 0; d < 4; d++) D[d] = deviation_from_bits(bits[d]);
  return MUGIQ_HIP_SUCCESS;
}

template <typename F>
static int build_axial_gauge_links_t(void *G_d, const MugiqHipSpinorField &ev, const MugiqHipGaugeField &U, int kmax, int dir, int sign, hipStream_t stream) {
  AxialLinkArgs<F> g;
  g.G = static_cast<Cplx<double> *>(G_d);
  g.U = static_cast<const Cplx<F> *>(U.data);
  g.Upo = U.parity_offset;
  g.Ustride = U.stride;
  for (int d = 0; d < 4; d++) {
    g.X[d] = ev.X[d];
    g.R[d] = U.R[d];
  }
  const LineGeometry lines = line_geometry(ev, dir);
  g.dir = dir;
  g.kmax = kmax;
  g.sign = sign;
  g.J = ev.X[dir];
  g.strideMu = lines.strideMu;
  g.H = lines.H;
  g.numCols = lines.numCols;
  g.rowMode = dir == 0;
  hipLaunchKernelGGL(axial_gauge_from_links_kernel<F>, dim3((g.numCols + 63) / 64), dim3(64), 0, stream, g);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}
int build_axial_gauge_from_links(void *G_d, const MugiqHipSpinorField &ev, const MugiqHipGaugeField &U, int kmax, int dir, int sign, hipStream_t stream) {
  MUGIQ_REQUIRE(axial_gauge_from_links_possible(ev, U, kmax, dir, sign, FusedSwitches{}), "axial gauge from the links: precision %d / border %d along %d, lengths up to %d (internal)", U.precision, U.R[dir], dir, kmax);
  return ev.precision == 8 ? build_axial_gauge_links_t<double>(G_d, ev, U, kmax, dir, sign, stream)
                           : build_axial_gauge_links_t<float>(G_d, ev, U, kmax, dir, sign, stream);
}

// ultra_d != NULL: also produce the ultra-local loop (k = 0) into ultra_d as one more slot; *carried says whether that
// happened (only a launch over the whole lattice may: see csrc/fused_tile.hip).  evL != NULL: the two-sided tile, evL the left set
// and ev the right (displaced) one
int mfma_tile_entry(const FusedForm &form, void *loop_d, const MugiqHipSpinorField *ev, const double *sigma, int nVec, const void *const *E_d,
                    const int *kvals, int nK, int sign, const void *ghost_d, int layers, int region,
                    hipStream_t stream, void *ultra_d, int *carried, const MugiqHipSpinorField *evL, const void *G_d,
                    const EntryPackTarget *pack, int nPack, bool *packed) {
  MUGIQ_REQUIRE(nPack <= kMT_MaxPack && (nPack == 0 || packed), "mfma tile: %d pack targets (internal)", nPack);
  const int dir = form.dir, partitioned = form.partitioned, loopPrecision = form.loopPrecision;
  const bool two = evL != nullptr;
  MTileArgs a;
  const void *invSigma = nullptr;
  int st = upload_vector_table(&a.L, &invSigma, ev, evL, sigma, nVec, 8, 8, stream);  // (1/sigma in double whatever the storage)
  if (st) return st;
  const int64_t slot_stride = (int64_t)16 * 2 * ev[0].volumeCB * 2 * loopPrecision;  // bytes
  a.outFloat = loopPrecision == 4;
  if (carried) *carried = 0;
  a.VL = two ? a.L + nVec : nullptr;
  a.inv_sigma = static_cast<const double *>(invSigma);
  a.nVec = nVec;
  for (int d = 0; d < 4; d++) a.X[d] = ev[0].X[d];
  a.volumeCB = ev[0].volumeCB;
  a.stride = ev[0].stride;
  a.parity_offset = ev[0].parity_offset;
  a.partitioned = partitioned;
  a.ghost = ghost_d;
  const LineGeometry lines = line_geometry(ev[0], dir, layers);
  a.faceCB = lines.faceCB;
  a.ghost_vec_stride = lines.ghost_vec_stride;
  a.strideMu = lines.strideMu;
  a.H = lines.H;
  a.numCols = lines.numCols;
  if (dir == 0) ultra_d = nullptr;  // (the row tile takes no fourth slot)
  a.overwrite = (region & MUGIQ_HIP_REGION_OVERWRITE) ? 1 : 0;
  region &= 0xff;
  if (region != MUGIQ_HIP_REGION_ALL) ultra_d = nullptr;
  a.kmaxG = kvals[nK - 1];  // (select_fused_form: ascending; 1 .. nK unless the caller's gauge is at hand)
  // the axial gauge of this (direction, sign): the caller's, if it has built one; else rebuilt into the stream's workspace (one
  // pass over W_1)
  if (G_d) {
    a.G = static_cast<const Cplx<double> *>(G_d);
  } else {
    void *gbuf = nullptr;
    if ((st = stream_workspace(&gbuf, form.gaugeBytes, stream))) return st;
    if ((st = build_axial_gauge(gbuf, ev[0], E_d, a.kmaxG, dir, sign, stream))) return st;
    a.G = static_cast<const Cplx<double> *>(gbuf);
  }
  // launches of up to four slots each (the first one may carry the ultra-local loop as its fourth); a launch of lengths
  // k0 .. k1 stages the TJ + k1 positions its sites and their shifted partners live on
  for (int first = 0, ns = 0; first < nK; first += ns) {
    const bool takesUltra = ultra_d && first == 0;
    ns = fused_even_slots(nK - first + (takesUltra ? 1 : 0), form.slotsPerLaunch) - (takesUltra ? 1 : 0);  // 1 .. 8 with the ultra-local loop = 3 + 3 + 3 slots
    a.kmax = kvals[first + ns - 1];
    for (int s = 0; s < kMT_MaxSlots; s++) {
      const int i = first + (s < ns ? s : 0);
      a.k[s] = kvals[i];
      a.out[s] = static_cast<char *>(loop_d) + (int64_t)i * slot_stride;
    }
    bool withUltra = false;
    int nSlots = ns;
    if (takesUltra) {
      a.k[nSlots] = 0;
      a.out[nSlots] = ultra_d;
      nSlots++;
      withUltra = true;
    }
    // the tile of THIS launch (its slots and the positions it stages; the gauge does not depend on it)
    const MfmaLaunch g = mfma_launch_geometry(form, nSlots, a.kmax);
    a.leftBufElems = g.leftBufElems;
    a.rowsPerTile = g.rows;
    a.rowChunk = g.rowChunk;
    a.nPack = 0;
    if (!two && dir == 0 && first == 0 && nPack > 0 && !*packed && ev[0].X[1] % a.rowsPerTile == 0) {  // the first launch of the entry packs
      a.nPack = nPack;
      for (int i = 0; i < nPack; i++) {
        const int fcb = ev[0].volumeCB / ev[0].X[pack[i].dim];
        a.pack[i].base = static_cast<Cplx<double> *>(pack[i].out_d);
        a.pack[i].dim = pack[i].dim;
        a.pack[i].high = pack[i].high;
        a.pack[i].layers = pack[i].layers;
        a.pack[i].from = pack[i].fromVec;
        a.pack[i].faceCB = fcb;
        a.pack[i].vecStride = (int64_t)pack[i].layers * 24 * fcb;
      }
      *packed = true;
    }
    // (the split is by the ENTRY's longest length, so that the interior and the boundary launch of a slot cover complementary tiles)
    tile_range(region, partitioned, sign, ev[0].X[dir] / g.tj, a.kmaxG, g.tj, a.jtBegin, a.jtCount);
    if (a.jtCount > 0) {
      st = launch_mfma_tile(a, ev[0].precision, ev[0].field_order, dir, sign, nSlots, g, stream);
      if (st) return st;
      if (withUltra && carried) *carried = 1;
    }
  }
  return MUGIQ_HIP_SUCCESS;
}

}  // namespace mugiq
