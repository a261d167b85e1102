// The Wilson and Wilson-clover operators on the fields this library already holds, and what rests on them: the eigenpair check of
// Eigsolve_Mugiq::computeEvals (host procedure and the five forms: csrc/op_forms.h), projectVector (lib/eigsolve_mugiq.cpp:340-348) and a
// CG on the normal equations started from the low-mode part.  Twisted-mass terms, the inverse clover term, even-odd preconditioning and mixed precision are out of scope.
//
//   M psi(x) = A(x) psi(x) - kappa sum_mu [ (1 - g_mu) U_mu(x) psi(x+mu) + (1 + g_mu) U_mu^dag(x-mu) psi(x-mu) ]
//   A = 1 (Wilson) | the clover term of a MugiqHipCloverField (csrc/clover.hip): two Hermitian 6 x 6 blocks per site, which commute with g5
//   g_x, g_y, g_z, g_t = Gamma_1, Gamma_2, Gamma_4, Gamma_8 of the library's table, g5 = Gamma_15 = diag(1, 1, -1, -1)
//
// Links are applied as stored (boundary phases, anisotropy: the host's business; no unitarity assumed).  M^dag = g5 M g5 is the same
// stencil with the sign of every g_mu flipped, so dagger and g5 are run-time flags of ONE kernel per storage type.
//
// wilson_kernel: one lattice site per lane, NB vectors per lane.  The loop over the eight hops is the outer one: a link is loaded
// once (18 reals) and applied to the NB neighbour spinors in turn, each projected to its two independent spin components first
// (1 -+ g_mu has rank 2: two SU(3) x vector products per hop instead of four; the other two components are a phase times the
// first two).  NB results (24 reals each) stay in registers across the hops; the diagonal term, kappa, g5 and the overall scale
// are folded in, nothing is written per direction.  NB = 4 for fp64 and 8 for fp32 fields: 192 accumulator registers either way,
// which with the link, one neighbour spinor and the index arithmetic fits the 512 registers a lane of a 2-wave workgroup may use
// without scratch (checked with -Rpass-analysis=kernel-resource-usage).
// CLOVER: the accumulators start as A(x) psi_v(x) instead of psi_v(x).  One packed block (36 reals) is loaded at a time and applied to the
// NB vectors; it is dead before the hops start.  A is Hermitian and commutes with g5, so the dagger and gamma5 flags need nothing more.
#include "op_forms.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace mugiq {
int validate_gauge(const MugiqHipGaugeField *U, const MugiqHipSpinorField *ref, const char *who);  // displace.hip
namespace {

constexpr int kWilsonThreads = 128;  // lanes (sites) per workgroup of the stencil
constexpr int kOpBlock = 8;          // vectors per halo transfer group, per reduction launch and per block of right-hand sides
constexpr int kRedThreads = 256;
constexpr int kRedMaxGroups = 1024;  // workgroups of a reduction: the partial sums a fixed-order final pass adds up
constexpr int kWilsonGamma[4] = {1, 2, 4, 8};

template <typename F> constexpr int wilson_nb() { return sizeof(F) == 8 ? 4 : 8; }

struct WilsonGeom {
  int X[4], XE[4], brd[4], part[4], faceCB[4];
  int volumeCB, stride, gstride;
  int64_t po, gpo;  // parity offsets (complex elements) of the spinors and of the gauge field
};

template <int NB> struct WilsonPtrs {
  const void *src[NB];
  void *dst[NB];
  const void *ghost[NB][4][2];
};

template <typename F, int ORDER>
__device__ inline void load12(Cplx<F> v[12], const void *base, int stride, int64_t po, int parity, int x_cb) {
  typedef F vec2 __attribute__((ext_vector_type(2)));
  typedef F vec4 __attribute__((ext_vector_type(4)));
  const vec2 *b2 = reinterpret_cast<const vec2 *>(base) + parity * po;
  if constexpr (ORDER == 2) {
    const MUGIQ_GLOBAL vec2 *p = as_global(b2) + x_cb;
#pragma unroll
    for (int k = 0; k < 12; k++) {
      const vec2 t = p[(int64_t)k * stride];
      v[k] = Cplx<F>{t.x, t.y};
    }
  } else {
    const MUGIQ_GLOBAL vec4 *p = as_global(reinterpret_cast<const vec4 *>(b2)) + x_cb;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const vec4 t = p[(int64_t)j * stride];
      v[2 * j] = Cplx<F>{t.x, t.y};
      v[2 * j + 1] = Cplx<F>{t.z, t.w};
    }
  }
}

template <typename F, int ORDER>
__device__ inline void store12(const Cplx<F> v[12], void *base, int stride, int64_t po, int parity, int x_cb) {
  typedef F vec2 __attribute__((ext_vector_type(2)));
  typedef F vec4 __attribute__((ext_vector_type(4)));
  vec2 *b2 = reinterpret_cast<vec2 *>(base) + parity * po;
  if constexpr (ORDER == 2) {
    MUGIQ_GLOBAL vec2 *p = as_global(b2) + x_cb;
#pragma unroll
    for (int k = 0; k < 12; k++) {
      vec2 t;
      t.x = v[k].re;
      t.y = v[k].im;
      p[(int64_t)k * stride] = t;
    }
  } else {
    MUGIQ_GLOBAL vec4 *p = as_global(reinterpret_cast<vec4 *>(b2)) + x_cb;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      vec4 t;
      t.x = v[2 * j].re;
      t.y = v[2 * j].im;
      t.z = v[2 * j + 1].re;
      t.w = v[2 * j + 1].im;
      p[(int64_t)j * stride] = t;
    }
  }
}

// i^ph * z
template <typename F> __device__ inline Cplx<F> mul_phase(int ph, const Cplx<F> &z) {
  switch (ph & 3) {
  case 0: return z;
  case 1: return Cplx<F>{-z.im, z.re};
  case 2: return Cplx<F>{-z.re, -z.im};
  default: return Cplx<F>{z.im, -z.re};
  }
}

// acc_v += -kappa (1 - sg g_DIR) W psi_v(x +- DIR),  W = U_DIR(x) (FWD) | U_DIR^dag(x - DIR),  sg = +-sgn (FWD | not), sgn = -1 for M^dag
template <typename F, int ORDER, typename FG, int NB, int DIR, int FWD>
__device__ inline void wilson_hop(Cplx<F> (&acc)[NB][12], const WilsonPtrs<NB> &P, const FG *U, const WilsonGeom &g, const int coord[4],
                                  int pty, int nv, F mkappa, F sgn) {
  typedef FG gvec2 __attribute__((ext_vector_type(2)));
  const int nbrPty = 1 - pty;
  int dx[4] = {0, 0, 0, 0};
  dx[DIR] = FWD ? 1 : -1;
  const bool offFace = g.part[DIR] && (FWD ? (coord[DIR] + 1 >= g.X[DIR]) : (coord[DIR] - 1 < 0));
  const int nidx = offFace ? ghost_face_index_on_face(coord, g.X, DIR) : link_index_shift(coord, dx, g.X);
  // the link from the extended field (as the displacement: lib/mugiq_displace_kernels.cu:39-66)
  int c2[4], dx1[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; i++) c2[i] = coord[i] + g.brd[i];
  if (!FWD) dx1[DIR] = -1;
  const int linkPty = FWD ? pty : 1 - pty;
  const int lidx = link_index_shift(c2, dx1, g.XE);
  Cplx<F> u[9];
  {
    const MUGIQ_GLOBAL gvec2 *p = as_global(reinterpret_cast<const gvec2 *>(U)) + linkPty * g.gpo + (int64_t)DIR * 9 * g.gstride + lidx;
    Cplx<F> w[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const gvec2 t = p[(int64_t)i * g.gstride];
      w[i] = Cplx<F>{(F)t.x, (F)t.y};
    }
    if (FWD) {
#pragma unroll
      for (int i = 0; i < 9; i++) u[i] = w[i];
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) u[i * 3 + j] = Cplx<F>{w[j * 3 + i].re, -w[j * 3 + i].im};
    }
  }
  const F sg = FWD ? sgn : -sgn;
  constexpr int G = kWilsonGamma[DIR];
#pragma unroll
  for (int v = 0; v < NB; v++) {
    if (v < nv) {
      Cplx<F> psi[12];
      if (offFace) load12<F, ORDER>(psi, P.ghost[v][DIR][FWD], g.faceCB[DIR], (int64_t)12 * g.faceCB[DIR], nbrPty, nidx);
      else load12<F, ORDER>(psi, P.src[v], g.stride, g.po, nbrPty, nidx);
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int ph = kGammaPhase[G][i], col = kGammaColumn[G][i];  // (g psi)_i = i^ph psi_col, col in {2, 3}
        Cplx<F> chi[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const Cplx<F> gp = mul_phase(ph, psi[col * 3 + c]);
          chi[c] = Cplx<F>{mkappa * (psi[i * 3 + c].re - sg * gp.re), mkappa * (psi[i * 3 + c].im - sg * gp.im)};
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
          Cplx<F> w{F(0), F(0)};
#pragma unroll
          for (int j = 0; j < 3; j++) cmadd(w, u[c * 3 + j], chi[j]);
          acc[v][i * 3 + c].re += w.re;
          acc[v][i * 3 + c].im += w.im;
          // component col of (1 - sg g) psi is -sg conj(i^ph) times component i
          const Cplx<F> l = mul_phase(4 - ph, w);
          acc[v][col * 3 + c].re -= sg * l.re;
          acc[v][col * 3 + c].im -= sg * l.im;
        }
      }
    }
  }
}

// the clover field of a launch (nothing for the unimproved operator)
template <bool CLOVER> struct CloverArg {};
template <> struct CloverArg<true> {
  const void *data;
  int stride;
  int64_t po;
};

// acc_v <- A(x) acc_v: block b of the packed field (3 pairs of diagonal reals, 15 strictly-lower entries, row by row) on spins 2b, 2b + 1
template <typename F, typename FG, int NB>
__device__ inline void clover_apply(Cplx<F> (&acc)[NB][12], const CloverArg<true> &C, int pty, int x_cb, int nv) {
  typedef FG cvec2 __attribute__((ext_vector_type(2)));
  const MUGIQ_GLOBAL cvec2 *p = as_global(reinterpret_cast<const cvec2 *>(C.data)) + pty * C.po + x_cb;
#pragma unroll
  for (int b = 0; b < 2; b++) {
    F d[6];
    Cplx<F> l[15];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const cvec2 t = p[(int64_t)(b * 18 + q) * C.stride];
      d[2 * q] = (F)t.x;
      d[2 * q + 1] = (F)t.y;
    }
#pragma unroll
    for (int k = 0; k < 15; k++) {
      const cvec2 t = p[(int64_t)(b * 18 + 3 + k) * C.stride];
      l[k] = Cplx<F>{(F)t.x, (F)t.y};
    }
#pragma unroll
    for (int v = 0; v < NB; v++) {
      if (v < nv) {
        Cplx<F> in[6], out[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
          in[i] = acc[v][b * 6 + i];
          out[i] = Cplx<F>{d[i] * in[i].re, d[i] * in[i].im};
        }
#pragma unroll
        for (int i = 1; i < 6; i++)
#pragma unroll
          for (int j = 0; j < i; j++) {
            const Cplx<F> a = l[i * (i - 1) / 2 + j];  // A_ij; A_ji = conj(A_ij)
            cmadd(out[i], a, in[j]);
            cmadd_conj(out[j], a, in[i]);
          }
#pragma unroll
        for (int i = 0; i < 6; i++) acc[v][b * 6 + i] = out[i];
      }
    }
  }
}

template <typename F, int ORDER, typename FG, int NB, bool CLOVER>
__global__ __launch_bounds__(kWilsonThreads) void wilson_kernel(WilsonPtrs<NB> P, const FG *U, WilsonGeom g, int nv, F kappa, F scale,
                                                                int dagger, int gamma5, CloverArg<CLOVER> C) {
  const int site = blockIdx.x * kWilsonThreads + threadIdx.x;
  if (site >= 2 * g.volumeCB) return;
  const int pty = site >= g.volumeCB ? 1 : 0;
  const int x_cb = site - pty * g.volumeCB;
  int coord[4];
  get_coords(coord, x_cb, g.X, pty);
  Cplx<F> acc[NB][12];
#pragma unroll
  for (int v = 0; v < NB; v++)
    if (v < nv) load12<F, ORDER>(acc[v], P.src[v], g.stride, g.po, pty, x_cb);
  if constexpr (CLOVER) clover_apply<F, FG, NB>(acc, C, pty, x_cb, nv);
  const F sgn = dagger ? F(-1) : F(1), mk = -kappa;
  wilson_hop<F, ORDER, FG, NB, 0, 1>(acc, P, U, g, coord, pty, nv, mk, sgn);
  wilson_hop<F, ORDER, FG, NB, 0, 0>(acc, P, U, g, coord, pty, nv, mk, sgn);
  wilson_hop<F, ORDER, FG, NB, 1, 1>(acc, P, U, g, coord, pty, nv, mk, sgn);
  wilson_hop<F, ORDER, FG, NB, 1, 0>(acc, P, U, g, coord, pty, nv, mk, sgn);
  wilson_hop<F, ORDER, FG, NB, 2, 1>(acc, P, U, g, coord, pty, nv, mk, sgn);
  wilson_hop<F, ORDER, FG, NB, 2, 0>(acc, P, U, g, coord, pty, nv, mk, sgn);
  wilson_hop<F, ORDER, FG, NB, 3, 1>(acc, P, U, g, coord, pty, nv, mk, sgn);
  wilson_hop<F, ORDER, FG, NB, 3, 0>(acc, P, U, g, coord, pty, nv, mk, sgn);
  const F lower = gamma5 ? -scale : scale;
#pragma unroll
  for (int v = 0; v < NB; v++)
    if (v < nv) {
#pragma unroll
      for (int k = 0; k < 12; k++) {
        const F s = k < 6 ? scale : lower;
        acc[v][k].re *= s;
        acc[v][k].im *= s;
      }
      store12<F, ORDER>(acc[v], P.dst[v], g.stride, g.po, pty, x_cb);
    }
}

// ---- vector algebra of the eigenpair check and of the solver: one site per lane, blockIdx.y = vector of the block -------------
struct VecArgs {
  const void *a[kOpBlock];
  const void *b[kOpBlock];
  void *c[kOpBlock];
  void *d[kOpBlock];
  double s[kOpBlock], s2[kOpBlock];
  unsigned active;
};
struct SiteGeom {
  int volumeCB, stride;
  int64_t po;
};

// the workgroup's sum of v[0..2] in a fixed order (tree over LDS) -> out[0..2]
__device__ inline void group_sum3(double v[3], double *out) {
  __shared__ double sh[3][kRedThreads];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 3; k++) sh[k][t] = v[k];
  __syncthreads();
  for (int s = kRedThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < 3; k++) sh[k][t] += sh[k][t + s];
    }
    __syncthreads();
  }
  if (t < 3) out[t] = sh[t][0];
}

// mode 0: (Re, Im) of sum conj(a) b and sum |a|^2;  mode 1: sum |(s + i s2) a - b|^2 in slot 0.  fp64 arithmetic for any storage.
template <typename F, int ORDER, int MODE>
__global__ __launch_bounds__(kRedThreads) void wilson_reduce_kernel(VecArgs A, SiteGeom g, double *partial) {
  const int v = blockIdx.y;
  if (!((A.active >> v) & 1u)) return;
  double acc[3] = {0.0, 0.0, 0.0};
  const double lr = A.s[v], li = A.s2[v];
  for (int site = blockIdx.x * kRedThreads + threadIdx.x; site < 2 * g.volumeCB; site += gridDim.x * kRedThreads) {
    const int pty = site >= g.volumeCB ? 1 : 0, x_cb = site - pty * g.volumeCB;
    Cplx<F> a[12], b[12];
    load12<F, ORDER>(a, A.a[v], g.stride, g.po, pty, x_cb);
    load12<F, ORDER>(b, A.b[v], g.stride, g.po, pty, x_cb);
#pragma unroll
    for (int k = 0; k < 12; k++) {
      const double ar = a[k].re, ai = a[k].im, br = b[k].re, bi = b[k].im;
      if (MODE == 0) {
        acc[0] = fma(ar, br, acc[0]);
        acc[0] = fma(ai, bi, acc[0]);
        acc[1] = fma(ar, bi, acc[1]);
        acc[1] = fma(-ai, br, acc[1]);
        acc[2] = fma(ar, ar, acc[2]);
        acc[2] = fma(ai, ai, acc[2]);
      } else {
        const double dr = lr * ar - li * ai - br, di = lr * ai + li * ar - bi;
        acc[0] = fma(dr, dr, acc[0]);
        acc[0] = fma(di, di, acc[0]);
      }
    }
  }
  group_sum3(acc, partial + ((size_t)v * gridDim.x + blockIdx.x) * 3);
}

// x (c) += alpha p (a);  r (d) -= alpha q (b);  |r|^2 of the workgroup's sites into slot 0
template <int ORDER> __global__ __launch_bounds__(kRedThreads) void cg_update_kernel(VecArgs A, SiteGeom g, double *partial) {
  const int v = blockIdx.y;
  if (!((A.active >> v) & 1u)) return;
  double acc[3] = {0.0, 0.0, 0.0};
  const double alpha = A.s[v];
  for (int site = blockIdx.x * kRedThreads + threadIdx.x; site < 2 * g.volumeCB; site += gridDim.x * kRedThreads) {
    const int pty = site >= g.volumeCB ? 1 : 0, x_cb = site - pty * g.volumeCB;
    Cplx<double> x[12], p[12];
    load12<double, ORDER>(x, A.c[v], g.stride, g.po, pty, x_cb);
    load12<double, ORDER>(p, A.a[v], g.stride, g.po, pty, x_cb);
#pragma unroll
    for (int k = 0; k < 12; k++) {
      x[k].re = fma(alpha, p[k].re, x[k].re);
      x[k].im = fma(alpha, p[k].im, x[k].im);
    }
    store12<double, ORDER>(x, A.c[v], g.stride, g.po, pty, x_cb);
    load12<double, ORDER>(x, A.d[v], g.stride, g.po, pty, x_cb);
    load12<double, ORDER>(p, A.b[v], g.stride, g.po, pty, x_cb);
#pragma unroll
    for (int k = 0; k < 12; k++) {
      x[k].re = fma(-alpha, p[k].re, x[k].re);
      x[k].im = fma(-alpha, p[k].im, x[k].im);
      acc[0] = fma(x[k].re, x[k].re, acc[0]);
      acc[0] = fma(x[k].im, x[k].im, acc[0]);
    }
    store12<double, ORDER>(x, A.d[v], g.stride, g.po, pty, x_cb);
  }
  group_sum3(acc, partial + ((size_t)v * gridDim.x + blockIdx.x) * 3);
}

// c = s a + s2 b on the sites (a or b NULL: that term is zero; c may be a or b)
template <int ORDER> __global__ __launch_bounds__(kRedThreads) void lincomb_kernel(VecArgs A, SiteGeom g) {
  const int v = blockIdx.y;
  if (!((A.active >> v) & 1u)) return;
  const double sa = A.s[v], sb = A.s2[v];
  for (int site = blockIdx.x * kRedThreads + threadIdx.x; site < 2 * g.volumeCB; site += gridDim.x * kRedThreads) {
    const int pty = site >= g.volumeCB ? 1 : 0, x_cb = site - pty * g.volumeCB;
    Cplx<double> o[12], t[12];
#pragma unroll
    for (int k = 0; k < 12; k++) o[k] = Cplx<double>{0.0, 0.0};
    if (A.a[v]) {
      load12<double, ORDER>(t, A.a[v], g.stride, g.po, pty, x_cb);
#pragma unroll
      for (int k = 0; k < 12; k++) o[k] = Cplx<double>{sa * t[k].re, sa * t[k].im};
    }
    if (A.b[v]) {
      load12<double, ORDER>(t, A.b[v], g.stride, g.po, pty, x_cb);
#pragma unroll
      for (int k = 0; k < 12; k++) {
        o[k].re = fma(sb, t[k].re, o[k].re);
        o[k].im = fma(sb, t[k].im, o[k].im);
      }
    }
    store12<double, ORDER>(o, A.c[v], g.stride, g.po, pty, x_cb);
  }
}

// out[v][k] = sum over the groups, in group order (0 for a vector that is not active)
__global__ void wilson_final_sum_kernel(const double *partial, int nGroups, unsigned active, double *out) {
  const int i = threadIdx.x;
  if (i >= kOpBlock * 3) return;
  const int v = i / 3, k = i - 3 * v;
  double s = 0.0;
  if ((active >> v) & 1u)
    for (int c = 0; c < nGroups; c++) s += partial[((size_t)v * nGroups + c) * 3 + k];
  out[i] = s;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
size_t body_bytes(const MugiqHipSpinorField &f, int prec) { return align256((size_t)2 * (size_t)f.parity_offset * 2 * (size_t)prec); }
size_t zone_bytes(const MugiqHipSpinorField &f, int prec, int d) { return (size_t)24 * (size_t)(f.volumeCB / f.X[d]) * 2 * (size_t)prec; }
size_t ghost_bytes(const MugiqHipSpinorField &f, int prec, const int part[4]) {
  size_t n = 0;
  for (int d = 0; d < 4; d++)
    if (part[d]) n += 2 * align256(zone_bytes(f, prec, d));
  return n;
}
// `count` fields laid out like `like` (precision prec, ghost zones on the partitioned axes) from *cur on
void carve_fields(unsigned char **cur, const MugiqHipSpinorField &like, int prec, const int part[4], int count, MugiqHipSpinorField *out) {
  for (int i = 0; i < count; i++) {
    out[i] = like;
    out[i].precision = prec;
    out[i].data = *cur;
    *cur += body_bytes(like, prec);
    for (int d = 0; d < 4; d++)
      for (int b = 0; b < 2; b++) {
        out[i].ghost[d][b] = nullptr;
        if (part[d]) {
          out[i].ghost[d][b] = *cur;
          *cur += align256(zone_bytes(like, prec, d));
        }
      }
  }
}

bool same_layout(const MugiqHipSpinorField &a, const MugiqHipSpinorField &b) {
  return same_geometry(a, b) && a.stride == b.stride && a.parity_offset == b.parity_offset;
}

}  // namespace

size_t stencil_send_bytes(const MugiqHipSpinorField &like, int prec, const int part[4], int n) { return (size_t)n * ghost_bytes(like, prec, part); }
size_t stencil_zone_bytes(const MugiqHipSpinorField &like, int prec, int d) { return align256(zone_bytes(like, prec, d)); }

int check_gauge(const MugiqHipGaugeField *U, const int X[4], const int part[4], const char *who) {
  MUGIQ_REQUIRE(U != nullptr && U->data != nullptr, "%s: gauge field is NULL", who);
  MUGIQ_REQUIRE(U->precision == 4 || U->precision == 8, "%s: gauge precision %d", who, U->precision);
  long long volEx = 1;
  int sumR = 0;
  for (int d = 0; d < 4; d++) {
    MUGIQ_REQUIRE(U->X[d] == X[d], "%s: gauge X[%d] = %d differs from the spinor's %d", who, d, U->X[d], X[d]);
    MUGIQ_REQUIRE(U->R[d] >= 0, "%s: gauge R[%d] = %d is negative", who, d, U->R[d]);
    MUGIQ_REQUIRE(!part[d] || U->R[d] >= 1, "%s: dimension %d is partitioned but the gauge field has no border along it (R = 0)", who, d);
    volEx *= U->X[d] + 2 * U->R[d];
    sumR += U->R[d];
  }
  MUGIQ_REQUIRE((sumR & 1) == 0, "%s: the sum of the gauge borders R must be even", who);
  MUGIQ_REQUIRE(U->stride >= volEx / 2, "%s: gauge stride %d < extended volumeCB %lld", who, U->stride, volEx / 2);
  MUGIQ_REQUIRE(U->parity_offset >= (int64_t)36 * U->stride, "%s: gauge parity_offset %lld < 36*stride", who, (long long)U->parity_offset);
  return MUGIQ_HIP_SUCCESS;
}

int check_comm(const MugiqHipComm *comm, int part[4], bool needSums, const char *who) {
  bool any = false;
  for (int d = 0; d < 4; d++) any |= (part[d] = comm_partitioned(comm, d) ? 1 : 0) != 0;
  if (comm) {
    MUGIQ_REQUIRE(comm->size >= 1 && comm->grid[3] >= 1, "%s: invalid comm (size %d)", who, comm->size);
    MUGIQ_REQUIRE(!any || comm->sendrecv != nullptr, "%s: comm->sendrecv is NULL", who);
    MUGIQ_REQUIRE(!(needSums && comm->size > 1) || (comm->reduce_space && comm->gather_time && comm->bcast), "%s: a comm callback is NULL", who);
  }
  return MUGIQ_HIP_SUCCESS;
}

namespace {

// the clover field of an operator call (NULL: none): geometry of the spinors, precision of the gauge field
int check_clover(const MugiqHipCloverField *C, const MugiqHipSpinorField &ref, const MugiqHipGaugeField *U, const char *who) {
  if (C == nullptr) return MUGIQ_HIP_SUCCESS;
  if (int st = validate_clover(C, ref.X, ref.volumeCB, who)) return st;
  MUGIQ_REQUIRE(C->precision == U->precision, "%s: clover precision %d differs from the gauge precision %d (the operator's precision)", who,
                C->precision, U->precision);
  return MUGIQ_HIP_SUCCESS;
}

// ghost zones of n fields on every partitioned axis: one transfer group
int exchange_block(const OpContext &c, const MugiqHipSpinorField *f, int n) {
  bool any = false;
  for (int d = 0; d < 4; d++) any |= c.part[d] != 0;
  if (!any) return MUGIQ_HIP_SUCCESS;
  const MugiqHipComm *comm = c.comm;
  int st;
  const bool grouped = comm->group_begin && comm->group_end;
  if (grouped && (st = comm->group_begin(comm->ctx))) return set_error(MUGIQ_HIP_ERROR_HIP, "%s: group_begin callback failed with status %d", c.who, st);
  unsigned char *send = c.send;
  for (int i = 0; i < n; i++)
    for (int d = 0; d < 4; d++) {
      if (!c.part[d]) continue;
      const size_t bytes = zone_bytes(f[i], f[i].precision, d);
      for (int high = 0; high < 2; high++) {
        if ((st = mugiq_hip_pack_face(send, &f[i], d, high, c.stream))) return st;
        if ((st = comm->sendrecv(comm->ctx, send, f[i].ghost[d][1 - high], bytes, d, high ? +1 : -1, c.stream)))
          return set_error(MUGIQ_HIP_ERROR_HIP, "%s: halo sendrecv callback failed with status %d", c.who, st);
        send += align256(bytes);
      }
    }
  if (grouped && (st = comm->group_end(comm->ctx, c.stream))) return set_error(MUGIQ_HIP_ERROR_HIP, "%s: group_end callback failed with status %d", c.who, st);
  return MUGIQ_HIP_SUCCESS;
}

template <typename F, int ORDER, typename FG, bool CLOVER>
int launch_stencil(const OpContext &c, const MugiqHipSpinorField *dst, const MugiqHipSpinorField *src, int n, int dagger, int gamma5, double scale) {
  constexpr int NB = wilson_nb<F>();
  WilsonGeom g;
  const MugiqHipSpinorField &s0 = src[0];
  for (int d = 0; d < 4; d++) {
    g.X[d] = s0.X[d];
    g.brd[d] = c.U->R[d];
    g.XE[d] = s0.X[d] + 2 * c.U->R[d];
    g.part[d] = c.part[d];
    g.faceCB[d] = s0.volumeCB / s0.X[d];
  }
  g.volumeCB = s0.volumeCB;
  g.stride = s0.stride;
  g.po = s0.parity_offset;
  g.gstride = c.U->stride;
  g.gpo = c.U->parity_offset;
  CloverArg<CLOVER> C;
  if constexpr (CLOVER) C = CloverArg<true>{c.clover->data, c.clover->stride, c.clover->parity_offset};
  const dim3 grid((2 * s0.volumeCB + kWilsonThreads - 1) / kWilsonThreads), block(kWilsonThreads);
  for (int v0 = 0; v0 < n; v0 += NB) {
    const int nv = std::min(NB, n - v0);
    WilsonPtrs<NB> P;
    for (int v = 0; v < NB; v++) {
      const int w = v0 + std::min(v, nv - 1);  // unused slots repeat the last vector (never dereferenced: v < nv guards)
      P.src[v] = src[w].data;
      P.dst[v] = dst[w].data;
      for (int d = 0; d < 4; d++)
        for (int b = 0; b < 2; b++) P.ghost[v][d][b] = src[w].ghost[d][b];
    }
    hipLaunchKernelGGL((wilson_kernel<F, ORDER, FG, NB, CLOVER>), grid, block, 0, c.stream, P, static_cast<const FG *>(c.U->data), g, nv,
                       (F)c.kappa, (F)scale, dagger, gamma5, C);
    MUGIQ_CHECK_HIP(hipGetLastError());
  }
  return MUGIQ_HIP_SUCCESS;
}

}  // namespace

int stencil_apply(const OpContext &c, const MugiqHipSpinorField *dst, const MugiqHipSpinorField *src, int n, int dagger, int gamma5, double scale) {
  if (n <= 0) return MUGIQ_HIP_SUCCESS;
  int st = exchange_block(c, src, n);
  if (st) return st;
  const int prec = src[0].precision, order = src[0].field_order, gp = c.U->precision;
  const bool clover = c.clover != nullptr;  // its precision is the gauge field's (check_clover)
#define MUGIQ_WILSON_CASE(P_, O_, F_)                                                                      \
  if (prec == P_ && order == O_) {                                                                         \
    if (clover)                                                                                            \
      return gp == 8 ? launch_stencil<F_, O_, double, true>(c, dst, src, n, dagger, gamma5, scale)         \
                     : launch_stencil<F_, O_, float, true>(c, dst, src, n, dagger, gamma5, scale);         \
    return gp == 8 ? launch_stencil<F_, O_, double, false>(c, dst, src, n, dagger, gamma5, scale)          \
                   : launch_stencil<F_, O_, float, false>(c, dst, src, n, dagger, gamma5, scale);          \
  }
  MUGIQ_WILSON_CASE(8, 2, double)
  MUGIQ_WILSON_CASE(8, 4, double)
  MUGIQ_WILSON_CASE(4, 2, float)
  MUGIQ_WILSON_CASE(4, 4, float)
#undef MUGIQ_WILSON_CASE
  return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: precision %d / field order %d", c.who, prec, order);
}

namespace {

// any form; tmp: n fields with ghost zones for the intermediate of the two normal operators
int apply_op(const OpContext &c, const MugiqHipSpinorField *dst, const MugiqHipSpinorField *src, int n, int opType, double scale,
             const MugiqHipSpinorField *tmp) {
  return apply_form(opType, [&c](auto... a) { return stencil_apply(c, a...); }, dst, src, tmp, n, scale);
}

int reduction_groups(const MugiqHipSpinorField &f) { return std::min(kRedMaxGroups, (2 * f.volumeCB + kRedThreads - 1) / kRedThreads); }
size_t reduction_bytes(const MugiqHipSpinorField &f) { return align256(sizeof(double) * 3 * kOpBlock * ((size_t)reduction_groups(f) + 1)); }

SiteGeom site_geom(const MugiqHipSpinorField &f) { return SiteGeom{f.volumeCB, f.stride, f.parity_offset}; }

// the sums of the last reduction launch, on the host and over all ranks: out[kOpBlock][3]
int fetch_sums(const OpContext &c, double *red_d, int nGroups, unsigned active, double out[kOpBlock * 3]) {
  double *res_d = red_d + (size_t)3 * kOpBlock * nGroups;
  hipLaunchKernelGGL(wilson_final_sum_kernel, dim3(1), dim3(64), 0, c.stream, red_d, nGroups, active, res_d);
  MUGIQ_CHECK_HIP(hipGetLastError());
  MUGIQ_CHECK_HIP(hipMemcpyAsync(out, res_d, sizeof(double) * kOpBlock * 3, hipMemcpyDeviceToHost, c.stream));
  MUGIQ_CHECK_HIP(hipStreamSynchronize(c.stream));
  if (c.comm && c.comm->size > 1) {
    std::vector<double> v(out, out + kOpBlock * 3);
    if (int st = sum_over_ranks(c.comm, v)) return st;
    std::copy(v.begin(), v.end(), out);
  }
  return MUGIQ_HIP_SUCCESS;
}

template <int MODE> int launch_reduce(const OpContext &c, const VecArgs &A, const MugiqHipSpinorField &f, int n, double *red_d) {
  const dim3 grid(reduction_groups(f), n), block(kRedThreads);
  const SiteGeom g = site_geom(f);
  if (f.precision == 8 && f.field_order == 2) hipLaunchKernelGGL((wilson_reduce_kernel<double, 2, MODE>), grid, block, 0, c.stream, A, g, red_d);
  else if (f.precision == 8) hipLaunchKernelGGL((wilson_reduce_kernel<double, 4, MODE>), grid, block, 0, c.stream, A, g, red_d);
  else if (f.field_order == 2) hipLaunchKernelGGL((wilson_reduce_kernel<float, 2, MODE>), grid, block, 0, c.stream, A, g, red_d);
  else hipLaunchKernelGGL((wilson_reduce_kernel<float, 4, MODE>), grid, block, 0, c.stream, A, g, red_d);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

// sum conj(a_i) b_i and |a_i|^2 -> out[i] = (re, im, norm2)
int dot_norm(const OpContext &c, const MugiqHipSpinorField *a, const MugiqHipSpinorField *b, int n, unsigned active, double *red_d,
             double out[kOpBlock * 3]) {
  VecArgs A{};
  for (int i = 0; i < n; i++) {
    A.a[i] = a[i].data;
    A.b[i] = b[i].data;
  }
  A.active = active;
  if (int st = launch_reduce<0>(c, A, a[0], n, red_d)) return st;
  return fetch_sums(c, red_d, reduction_groups(a[0]), active, out);
}

int lincomb(const OpContext &c, const MugiqHipSpinorField *dst, const MugiqHipSpinorField *a, const double *sa, const MugiqHipSpinorField *b,
            const double *sb, int n, unsigned active) {
  VecArgs A{};
  for (int i = 0; i < n; i++) {
    A.a[i] = a ? a[i].data : nullptr;
    A.b[i] = b ? b[i].data : nullptr;
    A.c[i] = dst[i].data;
    A.s[i] = sa ? sa[i] : 0.0;
    A.s2[i] = sb ? sb[i] : 0.0;
  }
  A.active = active;
  const dim3 grid(reduction_groups(dst[0]), n), block(kRedThreads);
  if (dst[0].field_order == 2) hipLaunchKernelGGL(lincomb_kernel<2>, grid, block, 0, c.stream, A, site_geom(dst[0]));
  else hipLaunchKernelGGL(lincomb_kernel<4>, grid, block, 0, c.stream, A, site_geom(dst[0]));
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

int copy_body(const MugiqHipSpinorField &dst, const MugiqHipSpinorField &src, hipStream_t stream) {
  const size_t bytes = (size_t)(src.parity_offset + (int64_t)12 * src.stride) * 2 * (size_t)src.precision;
  MUGIQ_CHECK_HIP(hipMemcpyAsync(dst.data, src.data, bytes, hipMemcpyDeviceToDevice, stream));
  return MUGIQ_HIP_SUCCESS;
}

int check_vector_set(const MugiqHipSpinorField *f, int n, const char *who, const char *name) {
  MUGIQ_REQUIRE(f != nullptr, "%s: %s is NULL", who, name);
  for (int i = 0; i < n; i++) {
    if (int st = validate_spinor(&f[i], who, name)) return st;
    MUGIQ_REQUIRE(same_layout(f[i], f[0]), "%s: %s vector %d differs in precision, field order, geometry, stride or parity offset from vector 0", who,
                  name, i);
  }
  return MUGIQ_HIP_SUCCESS;
}

}  // namespace
}  // namespace mugiq

using namespace mugiq;

// the three operator entries, for both operators (clover NULL: the unimproved one)
static int wilson_apply_impl(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec, const MugiqHipGaugeField *gauge,
                             const MugiqHipCloverField *clover, double kappa, int opType, double scale, const MugiqHipComm *comm, void *stream) {
  const char *who = "wilsonApply";
  MUGIQ_REQUIRE(dst_h != nullptr && src_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nVec >= 1, "%s: nVec = %d must be >= 1", who, nVec);
  MUGIQ_REQUIRE(valid_op(opType), "%s: opType %d is none of M, Mdag, MdagM, MMdag, H", who, opType);
  int st, part[4];
  if ((st = check_vector_set(src_h, nVec, who, "src"))) return st;
  if ((st = check_vector_set(dst_h, nVec, who, "dst"))) return st;
  MUGIQ_REQUIRE(same_layout(dst_h[0], src_h[0]), "%s: dst and src differ in precision, field order, geometry, stride or parity offset", who);
  if ((st = check_disjoint(dst_h, nVec, "dst", src_h, nVec, "src", who, false, " (the kernel reads neighbours of src)"))) return st;
  if ((st = check_comm(comm, part, false, who))) return st;
  if ((st = check_gauge(gauge, src_h[0].X, part, who))) return st;
  if ((st = check_clover(clover, src_h[0], gauge, who))) return st;
  for (int d = 0; d < 4; d++)
    for (int i = 0; part[d] && i < nVec; i++)
      MUGIQ_REQUIRE(src_h[i].ghost[d][0] != nullptr && src_h[i].ghost[d][1] != nullptr,
                    "%s: dimension %d is partitioned but src vector %d has no ghost zones for it", who, d, i);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  // workspace: [send buffers of a block][intermediate fields of a block, for the two normal operators]
  const int prec = src_h[0].precision;
  const size_t sendB = stencil_send_bytes(src_h[0], prec, part, kOpBlock);
  const size_t tmpB = normal_op(opType) ? (size_t)kOpBlock * (body_bytes(src_h[0], prec) + ghost_bytes(src_h[0], prec, part)) : 0;
  void *ws = nullptr;
  if ((st = stream_operator_workspace(&ws, sendB + tmpB + 256, s))) return st;
  OpContext c{gauge, comm, {part[0], part[1], part[2], part[3]}, kappa, s, static_cast<unsigned char *>(ws), who, clover};
  MugiqHipSpinorField tmp[kOpBlock];
  unsigned char *cur = c.send + sendB;
  if (tmpB) carve_fields(&cur, src_h[0], prec, part, kOpBlock, tmp);
  for (int v0 = 0; v0 < nVec; v0 += kOpBlock)
    if ((st = apply_op(c, dst_h + v0, src_h + v0, std::min(kOpBlock, nVec - v0), opType, scale, tmp))) return st;
  return MUGIQ_HIP_SUCCESS;
}

static int compute_evals_impl(const MugiqHipSpinorField *eVecs_h, int nEv, const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover,
                              double kappa, int opType, int massNormalization, double *lambda_h, double *residual_h, double *sigma_h,
                              const MugiqHipComm *comm, void *stream) {
  const char *who = "computeEvals";
  MUGIQ_REQUIRE(eVecs_h != nullptr && lambda_h != nullptr && residual_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nEv >= 1, "%s: nEv = %d must be >= 1", who, nEv);
  if (int rq = check_evals_request(opType, sigma_h, massNormalization, kappa, who)) return rq;
  int st, part[4];
  if ((st = check_vector_set(eVecs_h, nEv, who, "eVecs"))) return st;
  if ((st = check_comm(comm, part, true, who))) return st;
  if ((st = check_gauge(gauge, eVecs_h[0].X, part, who))) return st;
  if ((st = check_clover(clover, eVecs_h[0], gauge, who))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  // work memory: 3 blocks of kOpBlock vectors of the eigenvectors' storage (a copy with ghost zones, w = A v, the intermediate of a
  // normal operator), whatever nEv
  const MugiqHipSpinorField &e0 = eVecs_h[0];
  const int prec = e0.precision;
  const size_t sendB = stencil_send_bytes(e0, prec, part, kOpBlock);
  const size_t fieldB = body_bytes(e0, prec) + ghost_bytes(e0, prec, part);
  void *ws = nullptr;
  if ((st = stream_operator_workspace(&ws, sendB + 3 * kOpBlock * fieldB + reduction_bytes(e0) + 256, s))) return st;
  OpContext c{gauge, comm, {part[0], part[1], part[2], part[3]}, kappa, s, static_cast<unsigned char *>(ws), who, clover};
  MugiqHipSpinorField vc[kOpBlock], w[kOpBlock], tmp[kOpBlock];
  unsigned char *cur = c.send + sendB;
  carve_fields(&cur, e0, prec, part, kOpBlock, vc);
  carve_fields(&cur, e0, prec, part, kOpBlock, w);
  carve_fields(&cur, e0, prec, part, kOpBlock, tmp);
  double *red_d = reinterpret_cast<double *>(cur);
  const double scale = mass_scale(massNormalization, kappa);
  static_assert(kEvBlock == kOpBlock, "a block of the check is a block of the stencil and of the reductions");
  return check_eigenpairs(
      nEv, opType, lambda_h, residual_h, sigma_h,
      [&](int v0, int n) -> int {
        for (int i = 0; i < n; i++)
          if (int rc = copy_body(vc[i], eVecs_h[v0 + i], s)) return rc;
        return apply_op(c, w, vc, n, opType, scale, tmp);
      },
      [&](int, int n, double *sums) { return dot_norm(c, vc, w, n, (1u << n) - 1u, red_d, sums); },
      [&](int, int n, const double *lambda, double *sums) -> int {
        VecArgs A{};
        for (int i = 0; i < n; i++) {
          A.a[i] = vc[i].data;
          A.b[i] = w[i].data;
          A.s[i] = lambda[2 * i];
          A.s2[i] = lambda[2 * i + 1];
        }
        A.active = (1u << n) - 1u;
        if (int rc = launch_reduce<1>(c, A, vc[0], n, red_d)) return rc;
        return fetch_sums(c, red_d, reduction_groups(vc[0]), A.active, sums);
      });
}

extern "C" {

int mugiq_hip_project_vector(const MugiqHipSpinorField *out, const MugiqHipSpinorField *in, const MugiqHipSpinorField *eVecs_h, int nEv,
                             const MugiqHipComm *comm, void *stream) {
  const char *who = "projectVector";
  MUGIQ_REQUIRE(out != nullptr && in != nullptr && eVecs_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nEv >= 1, "%s: nEv = %d must be >= 1", who, nEv);
  int st;
  if ((st = validate_spinor(out, who, "out"))) return st;
  if ((st = validate_spinor(in, who, "in"))) return st;
  MUGIQ_REQUIRE(out->data != in->data, "%s: out and in must not alias", who);
  MUGIQ_REQUIRE(out->precision == 8, "%s: out must be an fp64 field", who);
  MUGIQ_REQUIRE(same_layout(*out, *in), "%s: out and in differ in precision, field order, geometry, stride or parity offset", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // out = 0 on the sites, then out -= sum_i v_i (-1)^-1 <v_i, in>: the overlap and update kernels of the deflation
  OpContext c{nullptr, comm, {0, 0, 0, 0}, 0.0, s, nullptr, who};
  if ((st = lincomb(c, out, nullptr, nullptr, nullptr, nullptr, 1, 1u))) return st;
  std::vector<double> minusOne((size_t)nEv, -1.0);
  return deflate_low_modes(out, in, 1, eVecs_h, minusOne.data(), nEv, 0, nullptr, comm, s, who);
}

}  // extern "C"

static int wilson_solve_impl(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                             const MugiqHipCloverField *clover, double kappa, const MugiqHipSpinorField *eVecs_h, const double *sigma_h, int nEv,
                             double tol, int maxIter, int *iters_out, double *relres_out, const MugiqHipComm *comm, void *stream) {
  const char *who = "wilsonSolve";
  MUGIQ_REQUIRE(x_h != nullptr && b_h != nullptr && iters_out != nullptr && relres_out != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nVec >= 1, "%s: nVec = %d must be >= 1", who, nVec);
  MUGIQ_REQUIRE(nEv >= 0 && (nEv == 0 || (eVecs_h != nullptr && sigma_h != nullptr)), "%s: nEv = %d with eVecs_h or sigma_h NULL", who, nEv);
  MUGIQ_REQUIRE(tol > 0.0 && maxIter >= 0, "%s: tol = %g must be positive and maxIter = %d non-negative", who, tol, maxIter);
  int st, part[4];
  if ((st = check_vector_set(b_h, nVec, who, "b"))) return st;
  if ((st = check_vector_set(x_h, nVec, who, "x"))) return st;
  MUGIQ_REQUIRE(b_h[0].precision == 8, "%s: x and b must be fp64 fields", who);
  MUGIQ_REQUIRE(same_layout(x_h[0], b_h[0]), "%s: x and b differ in precision, field order, geometry, stride or parity offset", who);
  if ((st = check_disjoint(x_h, nVec, "x", b_h, nVec, "b", who))) return st;
  std::vector<double> negSigma((size_t)nEv);
  for (int n = 0; n < nEv; n++) {
    MUGIQ_REQUIRE(sigma_h[n] != 0.0, "%s: sigma[%d] is zero", who, n);
    negSigma[n] = -sigma_h[n];
  }
  if (nEv && (st = check_vector_set(eVecs_h, nEv, who, "eVecs"))) return st;
  if ((st = check_comm(comm, part, true, who))) return st;
  if ((st = check_gauge(gauge, b_h[0].X, part, who))) return st;
  if ((st = check_clover(clover, b_h[0], gauge, who))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  // work memory: r, p, t = M p, q = M^dag t for a block of kOpBlock right-hand sides (fp64, with ghost zones), whatever nVec
  const MugiqHipSpinorField &b0 = b_h[0];
  const size_t sendB = stencil_send_bytes(b0, 8, part, kOpBlock);
  const size_t fieldB = body_bytes(b0, 8) + ghost_bytes(b0, 8, part);
  void *ws = nullptr;
  if ((st = stream_operator_workspace(&ws, sendB + 4 * kOpBlock * fieldB + reduction_bytes(b0) + 256, s))) return st;
  OpContext c{gauge, comm, {part[0], part[1], part[2], part[3]}, kappa, s, static_cast<unsigned char *>(ws), who, clover};
  MugiqHipSpinorField r[kOpBlock], p[kOpBlock], t[kOpBlock], q[kOpBlock];
  unsigned char *cur = c.send + sendB;
  carve_fields(&cur, b0, 8, part, kOpBlock, r);
  carve_fields(&cur, b0, 8, part, kOpBlock, p);
  carve_fields(&cur, b0, 8, part, kOpBlock, t);
  carve_fields(&cur, b0, 8, part, kOpBlock, q);
  double *red_d = reinterpret_cast<double *>(cur);
  const int nGroups = reduction_groups(b0);
  bool allConverged = true;
  double sums[kOpBlock * 3], one[kOpBlock], minus[kOpBlock];
  std::fill(one, one + kOpBlock, 1.0);
  std::fill(minus, minus + kOpBlock, -1.0);

  // the fields of `set` whose bit is set in `mask`, in order
  auto gather = [](const MugiqHipSpinorField *set, int n, unsigned mask, MugiqHipSpinorField *out) {
    int m = 0;
    for (int i = 0; i < n; i++)
      if ((mask >> i) & 1u) out[m++] = set[i];
    return m;
  };
  // q_i = M^dag M p_i for the active i (t_i = M p_i stays behind)
  auto normal = [&](int n, unsigned mask) -> int {
    MugiqHipSpinorField pa[kOpBlock], ta[kOpBlock], qa[kOpBlock];
    const int m = gather(p, n, mask, pa);
    gather(t, n, mask, ta);
    gather(q, n, mask, qa);
    if (int e = stencil_apply(c, ta, pa, m, 0, 0, 1.0)) return e;
    return stencil_apply(c, qa, ta, m, 1, 0, 1.0);
  };

  for (int v0 = 0; v0 < nVec; v0 += kOpBlock) {
    const int n = std::min(kOpBlock, nVec - v0);
    const unsigned all = (1u << n) - 1u;
    const MugiqHipSpinorField *x = x_h + v0, *b = b_h + v0;
    double bnorm2[kOpBlock], rhs2[kOpBlock], rr[kOpBlock], alpha[kOpBlock], beta[kOpBlock];
    // ||b||^2 and r = M^dag b
    if ((st = dot_norm(c, b, b, n, all, red_d, sums))) return st;
    for (int i = 0; i < n; i++) {
      bnorm2[i] = sums[3 * i + 2];
      if ((st = copy_body(p[i], b[i], s))) return st;
    }
    if ((st = stencil_apply(c, r, p, n, 1, 0, 1.0))) return st;
    if ((st = dot_norm(c, r, r, n, all, red_d, sums))) return st;
    for (int i = 0; i < n; i++) rhs2[i] = sums[3 * i + 2];
    // start vector: zero, or the low-mode part x0 = sum_n v_n sigma_n^-1 (v_n^dag g5 b), and then r -= M^dag M x0
    if ((st = lincomb(c, x, nullptr, nullptr, nullptr, nullptr, n, all))) return st;
    if (nEv > 0) {
      if ((st = deflate_low_modes(x, b, n, eVecs_h, negSigma.data(), nEv, 1, nullptr, comm, s, who))) return st;
      for (int i = 0; i < n; i++)
        if ((st = copy_body(p[i], x[i], s))) return st;
      if ((st = normal(n, all))) return st;
      if ((st = lincomb(c, r, r, one, q, minus, n, all))) return st;
      if ((st = dot_norm(c, r, r, n, all, red_d, sums))) return st;
    }
    unsigned active = 0;
    for (int i = 0; i < n; i++) {
      rr[i] = sums[3 * i + 2];
      iters_out[v0 + i] = 0;
      if (rhs2[i] > 0.0 && !(rr[i] <= tol * tol * rhs2[i])) active |= 1u << i;
      if ((st = copy_body(p[i], r[i], s))) return st;
    }
    for (int it = 0; it < maxIter && active; it++) {
      if ((st = normal(n, active))) return st;
      if ((st = dot_norm(c, t, t, n, active, red_d, sums))) return st;  // <p, M^dag M p> = ||M p||^2
      VecArgs A{};
      for (int i = 0; i < n; i++) {
        if (!((active >> i) & 1u)) continue;
        const double pAp = sums[3 * i + 2];
        if (!(pAp > 0.0)) {  // breakdown: p = 0
          active &= ~(1u << i);
          continue;
        }
        alpha[i] = rr[i] / pAp;
        A.a[i] = p[i].data;
        A.b[i] = q[i].data;
        A.c[i] = x[i].data;
        A.d[i] = r[i].data;
        A.s[i] = alpha[i];
      }
      if (!active) break;
      A.active = active;
      const dim3 grid(nGroups, n), block(kRedThreads);
      if (b0.field_order == 2) hipLaunchKernelGGL(cg_update_kernel<2>, grid, block, 0, s, A, site_geom(b0), red_d);
      else hipLaunchKernelGGL(cg_update_kernel<4>, grid, block, 0, s, A, site_geom(b0), red_d);
      MUGIQ_CHECK_HIP(hipGetLastError());
      if ((st = fetch_sums(c, red_d, nGroups, active, sums))) return st;
      unsigned next = active;
      for (int i = 0; i < n; i++) {
        if (!((active >> i) & 1u)) continue;
        iters_out[v0 + i]++;
        const double rrNew = sums[3 * i];
        beta[i] = rrNew / rr[i];
        rr[i] = rrNew;
        if (rrNew <= tol * tol * rhs2[i]) next &= ~(1u << i);
      }
      active = next;
      if (active && (st = lincomb(c, p, r, one, p, beta, n, active))) return st;  // p = r + beta p
    }
    // the true residual ||b - M x|| / ||b||, with one more application
    for (int i = 0; i < n; i++)
      if ((st = copy_body(p[i], x[i], s))) return st;
    if ((st = stencil_apply(c, t, p, n, 0, 0, 1.0))) return st;
    if ((st = lincomb(c, t, b, one, t, minus, n, all))) return st;
    if ((st = dot_norm(c, t, t, n, all, red_d, sums))) return st;
    for (int i = 0; i < n; i++) {
      relres_out[v0 + i] = bnorm2[i] > 0.0 ? std::sqrt(sums[3 * i + 2] / bnorm2[i]) : 0.0;
      if (rhs2[i] > 0.0 && !(rr[i] <= tol * tol * rhs2[i])) allConverged = false;
    }
  }
  if (!allConverged)
    return set_error(MUGIQ_HIP_ERROR_NOT_CONVERGED, "%s: not every right-hand side reached tol = %g within maxIter = %d (x, iters_out, relres_out are filled)",
                     who, tol, maxIter);
  return MUGIQ_HIP_SUCCESS;
}

extern "C" {

int mugiq_hip_wilson_apply(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec, const MugiqHipGaugeField *gauge,
                           double kappa, int opType, double scale, const MugiqHipComm *comm, void *stream) {
  return wilson_apply_impl(dst_h, src_h, nVec, gauge, nullptr, kappa, opType, scale, comm, stream);
}
int mugiq_hip_wilson_clover_apply(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec, const MugiqHipGaugeField *gauge,
                                  const MugiqHipCloverField *clover, double kappa, int opType, double scale, const MugiqHipComm *comm,
                                  void *stream) {
  return wilson_apply_impl(dst_h, src_h, nVec, gauge, clover, kappa, opType, scale, comm, stream);
}

int mugiq_hip_compute_evals(const MugiqHipSpinorField *eVecs_h, int nEv, const MugiqHipGaugeField *gauge, double kappa, int opType,
                            int massNormalization, double *lambda_h, double *residual_h, double *sigma_h, const MugiqHipComm *comm,
                            void *stream) {
  return compute_evals_impl(eVecs_h, nEv, gauge, nullptr, kappa, opType, massNormalization, lambda_h, residual_h, sigma_h, comm, stream);
}
int mugiq_hip_compute_evals_clover(const MugiqHipSpinorField *eVecs_h, int nEv, const MugiqHipGaugeField *gauge,
                                   const MugiqHipCloverField *clover, double kappa, int opType, int massNormalization, double *lambda_h,
                                   double *residual_h, double *sigma_h, const MugiqHipComm *comm, void *stream) {
  return compute_evals_impl(eVecs_h, nEv, gauge, clover, kappa, opType, massNormalization, lambda_h, residual_h, sigma_h, comm, stream);
}

int mugiq_hip_wilson_solve(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                           double kappa, const MugiqHipSpinorField *eVecs_h, const double *sigma_h, int nEv, double tol, int maxIter,
                           int *iters_out, double *relres_out, const MugiqHipComm *comm, void *stream) {
  return wilson_solve_impl(x_h, b_h, nVec, gauge, nullptr, kappa, eVecs_h, sigma_h, nEv, tol, maxIter, iters_out, relres_out, comm, stream);
}
int mugiq_hip_wilson_clover_solve(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                                  const MugiqHipCloverField *clover, double kappa, const MugiqHipSpinorField *eVecs_h, const double *sigma_h,
                                  int nEv, double tol, int maxIter, int *iters_out, double *relres_out, const MugiqHipComm *comm,
                                  void *stream) {
  return wilson_solve_impl(x_h, b_h, nVec, gauge, clover, kappa, eVecs_h, sigma_h, nEv, tol, maxIter, iters_out, relres_out, comm, stream);
}

}  // extern "C"
