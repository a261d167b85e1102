// Restriction R = P^dag, the adjoint of the prolongator of csrc/prolong.hip (QUDA Transfer::R), batched over right-hand sides, and
// the low-mode deflation of fine vectors THROUGH the coarse space of the MG hierarchy (eigsolve->computeCoarse: the eigenvectors
// w_n live on the coarsest level, v_n = P w_n is never stored):
//     coarse(X; S, j) = sum_{x in aggregate X} sum_{s: s / spin_bs = S} sum_c conj(V(x; s, c, j)) g(s) fine(x; s, c),   g = 1 | diag(g5)
//     dst_r <- dst_r - P [ sum_n w_n sigma_n^-1 c_nr ],   c_nr = <w_n, R(G src_r)>          (v_n^dag G src = w_n^dag R G src, exactly)
//
// Numerics (as csrc/deflate.hip): products and sums in fp64 whatever the storage, one rounding on the store, no atomics, and a
// summation order that depends on nothing but the shape of the transfer -- not on nVec, not on a vector's place in the batch.
//
// Finest level, restrict_kernel: a workgroup owns ONE aggregate and a block of kRsRB = 8 right-hand sides; V is read once per
// block and every element loaded is used for all eight.  256 lanes = 32 site slots x 8 null-vector groups: lane (slot, jg) walks
// the aggregate's sites slot, slot + 32, ... (coordinates -> parity, x_cb: odd block extents mix the parities site by site) and
// carries 3 null vectors j = jg, jg + 8, jg + 16 (more: further passes over the aggregate) x 8 right-hand sides = 24 fp64 complex
// accumulators per chirality.  The 32 slot partials of an output leave through LDS and are added in slot order by one lane.
// By the byte model HBM bound: 18 kflop per 4.6 KB of V at n_vec 24 is 4 flop/B, below the fp64 ridge -- the vector pipe, no MFMA.
// (Measured, DESIGN.md 4.4a: 3.4 x one read of V; the right-hand sides are re-loaded by all 8 groups of a site, V comes in 32-byte pieces.)
// Workgroups follow xcd_contiguous_block: x-adjacent aggregates share the 128-byte lines of a V row and run on one XCD.
// Coarse -> coarse levels (256 x smaller): restrict_coarse_kernel, one lane per coarse site, output component and eight vectors.
#include "mg_common.h"
#include "op_forms.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace mugiq {
namespace {

constexpr int kRsSlots = 32;  // fine sites of the aggregate in flight
constexpr int kRsJG = 8;      // null-vector groups (lanes per site)
constexpr int kRsJC = 3;      // null vectors per lane and pass
constexpr int kRsRB = 8;      // right-hand sides per workgroup
constexpr int kRsHalf = 4;    // right-hand sides per trip through LDS

// diag(g5), g5 = Gamma_15 of the DeGrand-Rossi tables (internal.h): diagonal with real entries
template <int S> constexpr double gamma5_entry() {
  static_assert(kGammaColumn[15][S] == S && (kGammaPhase[15][S] == 0 || kGammaPhase[15][S] == 2), "gamma5 must be diagonal and real");
  return kGammaPhase[15][S] == 0 ? 1.0 : -1.0;
}
__device__ inline double gamma5_diag(int s) {
  return s == 0 ? gamma5_entry<0>() : s == 1 ? gamma5_entry<1>() : s == 2 ? gamma5_entry<2>() : gamma5_entry<3>();
}

// complex element of component k = 3 s + c of a fine field body (SpinorView, internal.h)
template <int ORDER> __device__ inline int64_t fine_elem(int k, int pty, int x_cb, int stride, int64_t po) {
  if constexpr (ORDER == 2) return pty * po + (int64_t)k * stride + x_cb;
  else return pty * po + 2 * ((int64_t)(k >> 1) * stride + x_cb) + (k & 1);
}

struct RestrictArgs {
  const void *V;  // [parity][(3s+c)*NV + j][x_cb]
  int64_t Vpo;
  int Vstride, NV;
  TransferGeom g;
  const void *const *tab;  // device table: nVec fine bodies, then nVec coarse bodies
  int Fstride, Cstride;
  int64_t Fpo, Cpo;
  int nVec, gamma5;
};

template <typename FV, typename FS, int ORDER> __global__ __launch_bounds__(kRsSlots *kRsJG) void restrict_kernel(RestrictArgs a) {
  __shared__ Cplx<double> red[kRsJG * kRsJC * kRsHalf][kRsSlots + 1];
  const int t = threadIdx.x, slot = t & (kRsSlots - 1), jg = t / kRsSlots;
  int cc[4], r = xcd_contiguous_block(blockIdx.x, gridDim.x);
#pragma unroll
  for (int d = 0; d < 4; d++) {
    cc[d] = r % a.g.Xc[d];
    r /= a.g.Xc[d];
  }
  const int64_t coff = (int64_t)((cc[0] + cc[1] + cc[2] + cc[3]) & 1) * a.Cpo + (lex_index(cc, a.g.Xc) >> 1);
  const int n0 = blockIdx.y * kRsRB;
  const auto *tab = as_constant(a.tab);
  const void *fp[kRsRB];  // (vectors past the end shadow the last one; their sums are not stored)
#pragma unroll
  for (int i = 0; i < kRsRB; i++) fp[i] = tab[min(n0 + i, a.nVec - 1)];

  for (int j0 = 0; j0 < a.NV; j0 += kRsJG * kRsJC) {
    for (int chi = 0; chi < 2; chi++) {
      Cplx<double> acc[kRsJC][kRsRB];
#pragma unroll
      for (int i = 0; i < kRsJC; i++)
#pragma unroll
        for (int n = 0; n < kRsRB; n++) acc[i][n] = Cplx<double>{0.0, 0.0};
      for (int k = slot; k < a.g.aggVol; k += kRsSlots) {
        int pty, x_cb;
        aggregate_member(a.g.bs, a.g.X, cc, k, &pty, &x_cb);
        const int64_t voff = pty * a.Vpo + x_cb;
        for (int sc = 0; sc < 6; sc++) {
          const int comp = chi * 6 + sc;
          const double gs = a.gamma5 ? gamma5_diag(comp / 3) : 1.0;
          const int64_t fe = fine_elem<ORDER>(comp, pty, x_cb, a.Fstride, a.Fpo);
          Cplx<double> psi[kRsRB];
#pragma unroll
          for (int n = 0; n < kRsRB; n++) {
            const Cplx<double> p = ld_wide<FS>(fp[n], fe);
            psi[n] = Cplx<double>{gs * p.re, gs * p.im};
          }
#pragma unroll
          for (int i = 0; i < kRsJC; i++) {
            const int j = j0 + jg + kRsJG * i;
            if (j < a.NV) {
              const Cplx<double> v = ld_wide<FV>(a.V, voff + (int64_t)(comp * a.NV + j) * a.Vstride);
#pragma unroll
              for (int n = 0; n < kRsRB; n++) cmadd_conj(acc[i][n], v, psi[n]);
            }
          }
        }
      }
      // the 32 slot partials of every output, added in slot order
#pragma unroll
      for (int h = 0; h < kRsRB / kRsHalf; h++) {
        __syncthreads();  // the previous trip has been read
#pragma unroll
        for (int i = 0; i < kRsJC; i++)
#pragma unroll
          for (int nn = 0; nn < kRsHalf; nn++) red[(jg * kRsJC + i) * kRsHalf + nn][slot] = acc[i][h * kRsHalf + nn];
        __syncthreads();
        if (t < kRsJG * kRsJC * kRsHalf) {
          Cplx<double> s{0.0, 0.0};
          for (int q = 0; q < kRsSlots; q++) {
            s.re += red[t][q].re;
            s.im += red[t][q].im;
          }
          const int nn = t % kRsHalf, i = (t / kRsHalf) % kRsJC, jgo = t / (kRsHalf * kRsJC);
          const int j = j0 + jgo + kRsJG * i, n = n0 + h * kRsHalf + nn;
          if (j < a.NV && n < a.nVec) st_round<FV>(const_cast<void *>(tab[a.nVec + n]), coff + (int64_t)(chi * a.NV + j) * a.Cstride, s);
        }
      }
    }
  }
}

template <typename FV, typename FS, int ORDER>
int launch_restrict(const MugiqHipCoarseField *coarse, const MugiqHipSpinorField *fine, int nVec, const MugiqHipTransfer *T, int gamma5,
                    hipStream_t stream) {
  std::vector<const void *> host(2 * (size_t)nVec);
  for (int n = 0; n < nVec; n++) {
    host[n] = fine[n].data;
    host[nVec + n] = coarse[n].data;
  }
  void *dev = nullptr;
  if (int st = upload_table(&dev, host.data(), host.size() * sizeof(void *), stream)) return st;
  RestrictArgs a;
  a.V = T->V;
  a.Vpo = T->parity_offset;
  a.Vstride = T->stride;
  a.NV = T->nVec;
  a.g = transfer_geom(*T);
  a.tab = static_cast<const void *const *>(dev);
  a.Fstride = fine[0].stride;
  a.Fpo = fine[0].parity_offset;
  a.Cstride = coarse[0].stride;
  a.Cpo = coarse[0].parity_offset;
  a.nVec = nVec;
  a.gamma5 = gamma5 ? 1 : 0;
  const dim3 grid(2 * a.g.volumeCBc, (nVec + kRsRB - 1) / kRsRB);
  hipLaunchKernelGGL((restrict_kernel<FV, FS, ORDER>), grid, dim3(kRsSlots * kRsJG), 0, stream, a);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

int validate_restrict(const MugiqHipCoarseField *coarse_h, const MugiqHipSpinorField *fine_h, int nVec, const MugiqHipTransfer *T, const char *who) {
  MUGIQ_REQUIRE(fine_h && coarse_h && nVec >= 1, "%s: NULL / empty argument", who);
  int st = validate_transfer(T, &coarse_h[0], who);
  if (st) return st;
  for (int n = 0; n < nVec; n++) {
    if ((st = validate_spinor(&fine_h[n], who, "fine"))) return st;
    MUGIQ_REQUIRE(same_geometry(fine_h[n], fine_h[0]), "%s: fine field %d differs in precision, field order or geometry from field 0", who, n);
    MUGIQ_REQUIRE(coarse_h[n].data && coarse_h[n].stride == coarse_h[0].stride && coarse_h[n].parity_offset == coarse_h[0].parity_offset &&
                      coarse_h[n].precision == coarse_h[0].precision && coarse_h[n].nColor == coarse_h[0].nColor,
                  "%s: coarse field %d differs from field 0", who, n);
  }
  for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(fine_h[0].X[d] == T->X[d], "%s: fine X[%d] = %d, the transfer's is %d", who, d, fine_h[0].X[d], T->X[d]);
  return MUGIQ_HIP_SUCCESS;
}

// ---- coarse -> coarse levels ------------------------------------------------------------------------------------------------
// coarser(X; s, j) = sum_{x in X} sum_{c < nColor(finer)} conj(V(x; s, c, j)) finer(x; s, c): sites of the block in lexicographic
// order, colours ascending inside a site
struct RestrictCoarseArgs {
  const void *V;  // [parity][(NCf*s + c)*NV + j][x_cb]
  int64_t Vpo;
  int Vstride, NV, NCf;
  TransferGeom g;
  const void *const *tab;  // device table: nVec finer bodies, then nVec coarser bodies
  int Istride, Ostride;
  int64_t Ipo, Opo;
  int nVec;
};

template <typename F> __global__ __launch_bounds__(128) void restrict_coarse_kernel(RestrictCoarseArgs a) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= 2 * a.g.volumeCBc) return;
  const int cpar = tid / a.g.volumeCBc, xc_cb = tid - cpar * a.g.volumeCBc;
  const int k = blockIdx.y, s = k / a.NV, j = k - s * a.NV;  // output component (s, j)
  const int n0 = blockIdx.z * kRsRB;
  int cc[4];
  get_coords(cc, xc_cb, a.g.Xc, cpar);
  const auto *tab = as_constant(a.tab);
  const void *ip[kRsRB];
#pragma unroll
  for (int i = 0; i < kRsRB; i++) ip[i] = tab[min(n0 + i, a.nVec - 1)];
  Cplx<double> acc[kRsRB];
#pragma unroll
  for (int i = 0; i < kRsRB; i++) acc[i] = Cplx<double>{0.0, 0.0};
  for (int m = 0; m < a.g.aggVol; m++) {
    int pty, x_cb;
    aggregate_member(a.g.bs, a.g.X, cc, m, &pty, &x_cb);
    for (int c = 0; c < a.NCf; c++) {
      const int plane = s * a.NCf + c;
      const Cplx<double> v = ld_wide<F>(a.V, pty * a.Vpo + (int64_t)(plane * a.NV + j) * a.Vstride + x_cb);
      const int64_t ie = pty * a.Ipo + (int64_t)plane * a.Istride + x_cb;
#pragma unroll
      for (int i = 0; i < kRsRB; i++) cmadd_conj(acc[i], v, ld_wide<F>(ip[i], ie));
    }
  }
#pragma unroll
  for (int i = 0; i < kRsRB; i++)
    if (n0 + i < a.nVec) st_round<F>(const_cast<void *>(tab[a.nVec + n0 + i]), cpar * a.Opo + (int64_t)k * a.Ostride + xc_cb, acc[i]);
}

template <typename F>
int launch_restrict_coarse(const MugiqHipCoarseField *coarser, const MugiqHipCoarseField *finer, int nVec, const MugiqHipTransfer *T,
                           hipStream_t stream) {
  std::vector<const void *> host(2 * (size_t)nVec);
  for (int n = 0; n < nVec; n++) {
    host[n] = finer[n].data;
    host[nVec + n] = coarser[n].data;
  }
  void *dev = nullptr;
  if (int st = upload_table(&dev, host.data(), host.size() * sizeof(void *), stream)) return st;
  RestrictCoarseArgs a;
  a.V = T->V;
  a.Vpo = T->parity_offset;
  a.Vstride = T->stride;
  a.NV = T->nVec;
  a.NCf = finer[0].nColor;
  a.g = transfer_geom(*T);
  a.tab = static_cast<const void *const *>(dev);
  a.Istride = finer[0].stride;
  a.Ipo = finer[0].parity_offset;
  a.Ostride = coarser[0].stride;
  a.Opo = coarser[0].parity_offset;
  a.nVec = nVec;
  const dim3 grid((2 * a.g.volumeCBc + 127) / 128, 2 * a.NV, (nVec + kRsRB - 1) / kRsRB);
  hipLaunchKernelGGL((restrict_coarse_kernel<F>), grid, dim3(128), 0, stream, a);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

// ---- deflation through the coarse space ---------------------------------------------------------------------------------------
// Elements of a coarse field without its pads: e -> (parity, plane, x_cb), e < 2 * planes * volumeCB
struct CoarseGeom {
  int planes, volumeCB, stride;
  int64_t po;
  int nElem;
};
__device__ inline int64_t coarse_elem(const CoarseGeom &g, int e) {
  const int q = e / g.volumeCB, x = e - q * g.volumeCB;
  const int parity = q / g.planes, plane = q - parity * g.planes;
  return parity * g.po + (int64_t)plane * g.stride + x;
}

constexpr int kCoThreads = 256;
// C[n][r] = sum_e conj(w_n[e]) y_r[e] for the block r = r0 .. r0 + 7 of blockIdx.y: lane t adds e = t, t + 256, ... in ascending order,
// then the 256 lane sums are folded by a fixed halving tree in LDS.  D = C / sigma.
template <typename F>
__global__ __launch_bounds__(kCoThreads) void coarse_overlap_kernel(const void *const *W, const void *const *Y, int nVec, CoarseGeom g,
                                                                    const double *invSigma, Cplx<double> *C, Cplx<double> *D) {
  __shared__ Cplx<double> red[kRsRB][kCoThreads];
  const int n = blockIdx.x, r0 = blockIdx.y * kRsRB, t = threadIdx.x;
  const void *w = as_constant(W)[n];
  const void *yp[kRsRB];
#pragma unroll
  for (int i = 0; i < kRsRB; i++) yp[i] = as_constant(Y)[min(r0 + i, nVec - 1)];
  Cplx<double> acc[kRsRB];
#pragma unroll
  for (int i = 0; i < kRsRB; i++) acc[i] = Cplx<double>{0.0, 0.0};
  for (int e = t; e < g.nElem; e += kCoThreads) {
    const int64_t off = coarse_elem(g, e);
    const Cplx<double> wv = ld_wide<F>(w, off);
#pragma unroll
    for (int i = 0; i < kRsRB; i++) cmadd_conj(acc[i], wv, ld_wide<F>(yp[i], off));
  }
#pragma unroll
  for (int i = 0; i < kRsRB; i++) red[i][t] = acc[i];
  for (int s = kCoThreads / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) {
#pragma unroll
      for (int i = 0; i < kRsRB; i++) {
        red[i][t].re += red[i][t + s].re;
        red[i][t].im += red[i][t + s].im;
      }
    }
  }
  if (t < kRsRB && r0 + t < nVec) {
    const Cplx<double> c = red[t][0];
    C[(int64_t)n * nVec + r0 + t] = c;
    D[(int64_t)n * nVec + r0 + t] = Cplx<double>{c.re * invSigma[n], c.im * invSigma[n]};
  }
}

// z_r[e] = sum_n w_n[e] D[n][r], n ascending, for the block r = r0 .. r0 + 7 of blockIdx.y
template <typename F>
__global__ __launch_bounds__(kCoThreads) void coarse_combine_kernel(const void *const *W, void *const *Z, int nEv, int nVec, CoarseGeom g,
                                                                    const Cplx<double> *D) {
  const int e = blockIdx.x * kCoThreads + threadIdx.x, r0 = blockIdx.y * kRsRB;
  if (e >= g.nElem) return;
  const int64_t off = coarse_elem(g, e);
  Cplx<double> acc[kRsRB];
#pragma unroll
  for (int i = 0; i < kRsRB; i++) acc[i] = Cplx<double>{0.0, 0.0};
  for (int n = 0; n < nEv; n++) {
    const Cplx<double> wv = ld_wide<F>(as_constant(W)[n], off);
#pragma unroll
    for (int i = 0; i < kRsRB; i++) {
      typedef double vec2 __attribute__((ext_vector_type(2)));
      const vec2 d = *as_constant(reinterpret_cast<const vec2 *>(D) + (int64_t)n * nVec + min(r0 + i, nVec - 1));
      cmadd(acc[i], wv, Cplx<double>{d.x, d.y});
    }
  }
#pragma unroll
  for (int i = 0; i < kRsRB; i++)
    if (r0 + i < nVec) st_round<F>(as_constant(Z)[r0 + i], off, acc[i]);
}

// dst_r(x; s, c) -= sum_j V(x; s, c, j) z_r(X(x); s / 2, j), j ascending: the last prolongation and the update in one pass.  Lane =
// fine site (V rows coalesced along x_cb), blockIdx.y = component 3 s + c, blockIdx.z = block of eight right-hand sides: every V element
// is read once per block, every dst element read and written once
struct ProlongSubtractArgs {
  const void *V;
  int64_t Vpo;
  int Vstride, NV;
  TransferGeom g;
  const void *const *tab;  // device table: nVec coarse bodies (z), then nVec dst bodies
  int Fstride, Cstride;
  int64_t Fpo, Cpo;
  int nVec;
};
template <typename FV, typename FS, int ORDER> __global__ __launch_bounds__(128) void prolong_subtract_kernel(ProlongSubtractArgs a) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= 2 * a.g.volumeCB) return;
  const int pty = tid / a.g.volumeCB, x_cb = tid - pty * a.g.volumeCB;
  const int comp = blockIdx.y, chi = comp / 6, n0 = blockIdx.z * kRsRB;
  int c[4], cc[4];
  get_coords(c, x_cb, a.g.X, pty);
#pragma unroll
  for (int d = 0; d < 4; d++) cc[d] = c[d] / a.g.bs[d];
  const int64_t coff = (int64_t)((cc[0] + cc[1] + cc[2] + cc[3]) & 1) * a.Cpo + (lex_index(cc, a.g.Xc) >> 1) + (int64_t)(chi * a.NV) * a.Cstride;
  const auto *tab = as_constant(a.tab);
  const void *zp[kRsRB];
#pragma unroll
  for (int i = 0; i < kRsRB; i++) zp[i] = tab[min(n0 + i, a.nVec - 1)];
  Cplx<double> acc[kRsRB];
#pragma unroll
  for (int i = 0; i < kRsRB; i++) acc[i] = Cplx<double>{0.0, 0.0};
  const int64_t voff = pty * a.Vpo + (int64_t)comp * a.NV * a.Vstride + x_cb;
  for (int j = 0; j < a.NV; j++) {
    const Cplx<double> v = ld_wide<FV>(a.V, voff + (int64_t)j * a.Vstride);
#pragma unroll
    for (int i = 0; i < kRsRB; i++) cmadd(acc[i], v, ld_wide<FV>(zp[i], coff + (int64_t)j * a.Cstride));
  }
  const int64_t fe = fine_elem<ORDER>(comp, pty, x_cb, a.Fstride, a.Fpo);
#pragma unroll
  for (int i = 0; i < kRsRB; i++)
    if (n0 + i < a.nVec) {
      void *q = const_cast<void *>(tab[a.nVec + n0 + i]);
      const Cplx<double> d = ld_wide<FS>(q, fe);
      st_round<FS>(q, fe, Cplx<double>{d.re - acc[i].re, d.im - acc[i].im});
    }
}

template <typename FV, typename FS, int ORDER>
int launch_prolong_subtract(const MugiqHipSpinorField *dst, const MugiqHipCoarseField *z, int nVec, const MugiqHipTransfer *T, hipStream_t stream) {
  std::vector<const void *> host(2 * (size_t)nVec);
  for (int n = 0; n < nVec; n++) {
    host[n] = z[n].data;
    host[nVec + n] = dst[n].data;
  }
  void *dev = nullptr;
  if (int st = upload_table(&dev, host.data(), host.size() * sizeof(void *), stream)) return st;
  ProlongSubtractArgs a;
  a.V = T->V;
  a.Vpo = T->parity_offset;
  a.Vstride = T->stride;
  a.NV = T->nVec;
  a.g = transfer_geom(*T);
  a.tab = static_cast<const void *const *>(dev);
  a.Fstride = dst[0].stride;
  a.Fpo = dst[0].parity_offset;
  a.Cstride = z[0].stride;
  a.Cpo = z[0].parity_offset;
  a.nVec = nVec;
  const dim3 grid((2 * a.g.volumeCB + 127) / 128, 12, (nVec + kRsRB - 1) / kRsRB);
  hipLaunchKernelGGL((prolong_subtract_kernel<FV, FS, ORDER>), grid, dim3(128), 0, stream, a);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

int prolong_subtract(const MugiqHipSpinorField *dst, const MugiqHipCoarseField *z, int nVec, const MugiqHipTransfer *T, hipStream_t s) {
  const int pv = T->precision, pf = dst[0].precision, o = dst[0].field_order;
#define MUGIQ_PS_CASE(PV_, PF_, O_, FV_, FS_) \
  if (pv == PV_ && pf == PF_ && o == O_) return launch_prolong_subtract<FV_, FS_, O_>(dst, z, nVec, T, s);
  MUGIQ_PS_CASE(8, 8, 2, double, double)
  MUGIQ_PS_CASE(8, 8, 4, double, double)
  MUGIQ_PS_CASE(8, 4, 2, double, float)
  MUGIQ_PS_CASE(8, 4, 4, double, float)
  MUGIQ_PS_CASE(4, 8, 2, float, double)
  MUGIQ_PS_CASE(4, 8, 4, float, double)
  MUGIQ_PS_CASE(4, 4, 2, float, float)
  MUGIQ_PS_CASE(4, 4, 4, float, float)
#undef MUGIQ_PS_CASE
  return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "deflateLowModesCoarse: precision %d / %d, field order %d", pv, pf, o);
}

// The hierarchy of a call on coarse eigenvectors: transfers[0 .. nLevels) (finest first) fit together and the nEv eigenvectors live on
// the coarsest level.  lev[l]: the layout of the work vectors on level l + 1 (the coarser side of transfers[l]), without a body; the
// coarsest one takes the eigenvectors' stride and parity offset, so that one element offset serves both
int validate_hierarchy(const MugiqHipTransfer *transfers, int nLevels, const MugiqHipCoarseField *ev, int nEv, std::vector<MugiqHipCoarseField> *levOut,
                       const char *who) {
  int st;
  std::vector<MugiqHipCoarseField> &lev = *levOut;
  lev.assign(nLevels, MugiqHipCoarseField{});
  // level l + 1 fields (the coarser side of transfers[l]) as descriptors without data; lev[nLevels - 1] describes the eigenvectors
  for (int l = 0; l < nLevels; l++) {
    const MugiqHipTransfer &T = transfers[l];
    MUGIQ_REQUIRE(T.V != nullptr && T.nVec >= 1, "%s: transfer %d is empty", who, l);
    MUGIQ_REQUIRE(T.precision == ev[0].precision, "%s: transfer %d has precision %d, the eigenvectors %d", who, l, T.precision, ev[0].precision);
    for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(T.X[d] > 0 && T.geoBlockSize[d] >= 1, "%s: transfer %d: X / geo_block_size[%d]", who, l, d);
    lev[l] = coarse_side_layout(T);
    lev[l].data = reinterpret_cast<void *>(uintptr_t(16) * (l + 1));  // geometry only: the validators want distinct non-NULL bodies and never read them
    if (l == 0) st = validate_transfer(&T, &lev[0], who);
    else st = validate_coarse_transfer(&T, &lev[l - 1], &lev[l], 1, who);
    if (st) return st;
  }
  const MugiqHipCoarseField top = lev[nLevels - 1];
  for (int n = 0; n < nEv; n++) {
    const MugiqHipCoarseField &w = ev[n];
    MUGIQ_REQUIRE(w.data && w.precision == top.precision && w.nSpin == 2 && w.nColor == top.nColor && w.volumeCB == top.volumeCB,
                  "%s: coarse eigenvector %d does not live on the coarsest level (precision %d, nSpin 2, nColor %d, volumeCB %d)", who, n,
                  top.precision, top.nColor, top.volumeCB);
    for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(w.X[d] == top.X[d], "%s: coarse eigenvector %d: X[%d] = %d, expected %d", who, n, d, w.X[d], top.X[d]);
    MUGIQ_REQUIRE(w.stride >= w.volumeCB && w.parity_offset >= (int64_t)2 * w.nColor * w.stride && w.stride == ev[0].stride &&
                      w.parity_offset == ev[0].parity_offset, "%s: coarse eigenvector %d: stride / parity_offset", who, n);
  }
  lev[nLevels - 1].stride = ev[0].stride;  // the coarsest work vectors take the eigenvectors' layout: one element offset for both
  lev[nLevels - 1].parity_offset = ev[0].parity_offset;
  return MUGIQ_HIP_SUCCESS;
}

}  // namespace

int restrict_batched(const MugiqHipCoarseField *coarse, const MugiqHipSpinorField *fine, int nVec, const MugiqHipTransfer *T, int gamma5,
                     hipStream_t s) {
  const int pv = T->precision, pf = fine[0].precision, o = fine[0].field_order;
#define MUGIQ_RS_CASE(PV_, PF_, O_, FV_, FS_) \
  if (pv == PV_ && pf == PF_ && o == O_) return launch_restrict<FV_, FS_, O_>(coarse, fine, nVec, T, gamma5, s);
  MUGIQ_RS_CASE(8, 8, 2, double, double)
  MUGIQ_RS_CASE(8, 8, 4, double, double)
  MUGIQ_RS_CASE(8, 4, 2, double, float)
  MUGIQ_RS_CASE(8, 4, 4, double, float)
  MUGIQ_RS_CASE(4, 8, 2, float, double)
  MUGIQ_RS_CASE(4, 8, 4, float, double)
  MUGIQ_RS_CASE(4, 4, 2, float, float)
  MUGIQ_RS_CASE(4, 4, 4, float, float)
#undef MUGIQ_RS_CASE
  return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "restrictVecs: precision %d / %d, field order %d", pv, pf, o);
}

int restrict_coarse_batched(const MugiqHipCoarseField *coarser, const MugiqHipCoarseField *finer, int nVec, const MugiqHipTransfer *T,
                            hipStream_t s) {
  if (T->precision == 8) return launch_restrict_coarse<double>(coarser, finer, nVec, T, s);
  return launch_restrict_coarse<float>(coarser, finer, nVec, T, s);
}

int deflate_low_modes_coarse(const MugiqHipSpinorField *dst, const MugiqHipSpinorField *src, int nVec, const MugiqHipCoarseField *ev,
                             const double *sigma, int nEv, const MugiqHipTransfer *transfers, int nLevels, int gamma5, double *overlaps_h,
                             const MugiqHipComm *comm, hipStream_t stream, const char *who) {
  // ---- validation, before any device work
  MUGIQ_REQUIRE(dst != nullptr && src != nullptr && ev != nullptr && transfers != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nVec >= 1, "%s: nVec = %d must be >= 1", who, nVec);
  MUGIQ_REQUIRE(nEv >= 1, "%s: nEv = %d must be >= 1", who, nEv);
  MUGIQ_REQUIRE(nLevels >= 1 && nLevels <= 8, "%s: nCoarseLevels = %d must be in [1, 8]", who, nLevels);
  int st;
  std::vector<MugiqHipCoarseField> lev;
  if ((st = validate_hierarchy(transfers, nLevels, ev, nEv, &lev, who))) return st;
  const MugiqHipCoarseField top = lev[nLevels - 1];
  for (int n = 0; n < nEv; n++) MUGIQ_REQUIRE(sigma == nullptr || sigma[n] != 0.0, "%s: sigma[%d] is zero", who, n);
  for (int r = 0; r < nVec; r++) {
    if ((st = validate_spinor(&src[r], who, "src"))) return st;
    if ((st = validate_spinor(&dst[r], who, "dst"))) return st;
    MUGIQ_REQUIRE(same_geometry(src[r], src[0]) && same_geometry(dst[r], src[0]),
                  "%s: src / dst vector %d differs in precision, field order or geometry from src vector 0", who, r);
  }
  for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(src[0].X[d] == transfers[0].X[d], "%s: src X[%d] = %d, the finest transfer's is %d", who, d, src[0].X[d], transfers[0].X[d]);
  if ((st = check_disjoint(dst, nVec, "dst", src, nVec, "src", who, true, " without being identical to it"))) return st;
  const bool multi = comm != nullptr && comm->size > 1;
  if (comm) {
    MUGIQ_REQUIRE(comm->size >= 1 && comm->grid[3] >= 1, "%s: invalid comm (size %d)", who, comm->size);
    MUGIQ_REQUIRE(!multi || (comm->reduce_space && comm->gather_time && comm->bcast), "%s: a comm callback is NULL", who);
  }

  // ---- setup.  Workspace: nVec coarse vectors on every level, then C and D ([nEv][nVec] complex doubles each)
  if ((st = debug_poison_lds_if_asked(stream))) return st;
  const size_t P = (size_t)top.precision;
  std::vector<size_t> levOff(nLevels);
  size_t bytes = 0;
  for (int l = 0; l < nLevels; l++) {
    levOff[l] = bytes;
    bytes += align256((size_t)2 * lev[l].parity_offset * 2 * P * nVec);
  }
  const size_t cN = (size_t)nEv * nVec, cOff = bytes;
  bytes += 2 * cN * sizeof(Cplx<double>);
  void *ws = nullptr;
  if ((st = stream_workspace(&ws, bytes, stream))) return st;
  std::vector<std::vector<MugiqHipCoarseField>> y(nLevels, std::vector<MugiqHipCoarseField>(nVec));
  for (int l = 0; l < nLevels; l++)
    for (int r = 0; r < nVec; r++) {
      y[l][r] = lev[l];
      y[l][r].data = static_cast<unsigned char *>(ws) + levOff[l] + (size_t)r * 2 * lev[l].parity_offset * 2 * P;
    }
  Cplx<double> *C = reinterpret_cast<Cplx<double> *>(static_cast<unsigned char *>(ws) + cOff), *D = C + cN;

  // ---- c = <w, R G src>: all of src is read before any dst is written (src may alias dst)
  if ((st = restrict_batched(y[0].data(), src, nVec, &transfers[0], gamma5, stream))) return st;
  for (int l = 1; l < nLevels; l++)
    if ((st = restrict_coarse_batched(y[l].data(), y[l - 1].data(), nVec, &transfers[l], stream))) return st;
  // device tables: [eigenvector pointers][coarsest work vectors][1/sigma]
  const size_t pv = sizeof(void *) * (size_t)nEv, py = sizeof(void *) * (size_t)nVec;
  std::vector<unsigned char> host(pv + py + sizeof(double) * (size_t)nEv);
  const void **hw = reinterpret_cast<const void **>(host.data());
  void **hy = reinterpret_cast<void **>(host.data() + pv);
  double *hi = reinterpret_cast<double *>(host.data() + pv + py);
  for (int n = 0; n < nEv; n++) {
    hw[n] = ev[n].data;
    hi[n] = sigma ? 1.0 / sigma[n] : 1.0;
  }
  const std::vector<MugiqHipCoarseField> &yt = y[nLevels - 1];
  for (int r = 0; r < nVec; r++) hy[r] = yt[r].data;
  void *tab = nullptr;
  if ((st = upload_table(&tab, host.data(), host.size(), stream))) return st;
  const void *const *W_d = static_cast<const void *const *>(tab);
  void *const *Y_d = reinterpret_cast<void *const *>(static_cast<unsigned char *>(tab) + pv);
  const double *inv_d = reinterpret_cast<const double *>(static_cast<unsigned char *>(tab) + pv + py);
  const CoarseGeom g{2 * top.nColor, top.volumeCB, ev[0].stride, ev[0].parity_offset, 2 * 2 * top.nColor * top.volumeCB};
  const int nBlocks = (nVec + kRsRB - 1) / kRsRB;
  if (P == 8) hipLaunchKernelGGL((coarse_overlap_kernel<double>), dim3(nEv, nBlocks), dim3(kCoThreads), 0, stream, W_d, Y_d, nVec, g, inv_d, C, D);
  else hipLaunchKernelGGL((coarse_overlap_kernel<float>), dim3(nEv, nBlocks), dim3(kCoThreads), 0, stream, W_d, Y_d, nVec, g, inv_d, C, D);
  MUGIQ_CHECK_HIP(hipGetLastError());
  // ---- global overlaps: one synchronisation when they leave the device
  if (multi || overlaps_h) {
    std::vector<double> c(2 * cN);
    MUGIQ_CHECK_HIP(hipMemcpyAsync(c.data(), C, sizeof(Cplx<double>) * cN, hipMemcpyDeviceToHost, stream));
    MUGIQ_CHECK_HIP(hipStreamSynchronize(stream));
    if (multi) {
      if ((st = sum_over_ranks(comm, c))) return st;
      std::vector<double> d(2 * cN);
      for (int n = 0; n < nEv; n++)
        for (int r = 0; r < 2 * nVec; r++) d[(size_t)n * 2 * nVec + r] = c[(size_t)n * 2 * nVec + r] * hi[n];
      MUGIQ_CHECK_HIP(hipMemcpyAsync(D, d.data(), sizeof(Cplx<double>) * cN, hipMemcpyHostToDevice, stream));
      MUGIQ_CHECK_HIP(hipStreamSynchronize(stream));  // d is pageable and goes out of scope
    }
    if (overlaps_h) std::copy(c.begin(), c.end(), overlaps_h);
  }
  // ---- z = sum_n w_n sigma_n^-1 c_n on the coarsest level (over the restricted vectors), up the hierarchy, off dst
  const dim3 cgrid((g.nElem + kCoThreads - 1) / kCoThreads, nBlocks);
  if (P == 8) hipLaunchKernelGGL((coarse_combine_kernel<double>), cgrid, dim3(kCoThreads), 0, stream, W_d, Y_d, nEv, nVec, g, D);
  else hipLaunchKernelGGL((coarse_combine_kernel<float>), cgrid, dim3(kCoThreads), 0, stream, W_d, Y_d, nEv, nVec, g, D);
  MUGIQ_CHECK_HIP(hipGetLastError());
  for (int l = nLevels - 1; l >= 1; l--) {
    if ((st = debug_poison_lds_if_asked(stream))) return st;
    if ((st = prolong_coarse_batched(y[l - 1].data(), y[l].data(), nVec, &transfers[l], stream))) return st;
  }
  return prolong_subtract(dst, y[0].data(), nVec, &transfers[0], stream);
}

// ---- the eigenpair check on the coarsest level (check_eigenpairs of csrc/op_forms.h with the scalars below) ---------------------------
namespace {

// MODE 0: out[i] = (Re, Im <w_i, y_i>, |w_i|^2);  MODE 1: out[i] = (|lambda_i w_i - y_i|^2, 0, 0).  One workgroup per vector: lane t adds
// the elements t, t + 256, ... in ascending order, then a fixed halving tree in LDS
template <typename F, int MODE>
__global__ __launch_bounds__(kCoThreads) void coarse_scalar_kernel(const void *const *W, const void *const *Y, CoarseGeom g, const double *lambda,
                                                                   double *out) {
  __shared__ double red[3][kCoThreads];
  const int i = blockIdx.x, t = threadIdx.x;
  const void *w = as_constant(W)[i], *y = as_constant(Y)[i];
  const double lr = MODE == 1 ? lambda[2 * i] : 0.0, li = MODE == 1 ? lambda[2 * i + 1] : 0.0;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int e = t; e < g.nElem; e += kCoThreads) {
    const int64_t off = coarse_elem(g, e);
    const Cplx<double> wv = ld_wide<F>(w, off), yv = ld_wide<F>(y, off);
    if constexpr (MODE == 0) {
      a0 = fma(wv.re, yv.re, a0);
      a0 = fma(wv.im, yv.im, a0);
      a1 = fma(wv.re, yv.im, a1);
      a1 = fma(-wv.im, yv.re, a1);
      a2 = fma(wv.re, wv.re, a2);
      a2 = fma(wv.im, wv.im, a2);
    } else {
      const double dr = fma(lr, wv.re, fma(-li, wv.im, -yv.re)), di = fma(lr, wv.im, fma(li, wv.re, -yv.im));
      a0 = fma(dr, dr, a0);
      a0 = fma(di, di, a0);
    }
  }
  red[0][t] = a0, red[1][t] = a1, red[2][t] = a2;
  for (int s = kCoThreads / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s)
#pragma unroll
      for (int k = 0; k < 3; k++) red[k][t] += red[k][t + s];
  }
  if (t < 3) out[3 * i + t] = red[t][0];
}

// The sums of coarse_scalar_kernel<.., mode> over the pairs (w_i, y_i), i < n, of one layout, on the host and over all ranks of comm (NULL:
// this rank's).  scal_d: lambda of the block [2 kEvBlock], then the sums [3 kEvBlock].  Synchronises the stream
int coarse_scalars(int mode, const MugiqHipCoarseField *w, const MugiqHipCoarseField *y, int n, double *scal_d, const MugiqHipComm *comm,
                   hipStream_t stream, double out[3 * kEvBlock]) {
  std::vector<const void *> host(2 * (size_t)n);
  for (int i = 0; i < n; i++) host[i] = w[i].data, host[n + i] = y[i].data;
  void *tab = nullptr;
  if (int rc = upload_table(&tab, host.data(), host.size() * sizeof(void *), stream)) return rc;
  const void *const *W_d = static_cast<const void *const *>(tab);
  const CoarseGeom cg{2 * w[0].nColor, w[0].volumeCB, w[0].stride, w[0].parity_offset, 2 * 2 * w[0].nColor * w[0].volumeCB};
  double *sums_d = scal_d + 2 * kEvBlock;
  with_storage(w[0].precision, [&](auto f) {
    using F = decltype(f);
    hipLaunchKernelGGL((mode == 0 ? coarse_scalar_kernel<F, 0> : coarse_scalar_kernel<F, 1>), dim3(n), dim3(kCoThreads), 0, stream, W_d, W_d + n, cg,
                       scal_d, sums_d);
  });
  MUGIQ_CHECK_HIP(hipGetLastError());
  MUGIQ_CHECK_HIP(hipMemcpyAsync(out, sums_d, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, stream));
  MUGIQ_CHECK_HIP(hipStreamSynchronize(stream));
  if (comm && comm->size > 1) {
    std::vector<double> v(out, out + 3 * n);
    if (int rc = sum_over_ranks(comm, v)) return rc;
    std::copy(v.begin(), v.end(), out);
  }
  return MUGIQ_HIP_SUCCESS;
}

// The check of ev[0 .. nEv) with y_i = A_c w_i from apply(Y, w, n), block by block.  Y: kEvBlock work vectors laid out like the
// eigenvectors; scal_d: as above
template <typename Apply>
int check_coarse_eigenpairs(const MugiqHipCoarseField *ev, int nEv, int opType, const MugiqHipCoarseField *Y, double *scal_d, double *lambda_h,
                            double *residual_h, double *sigma_h, const MugiqHipComm *comm, hipStream_t stream, Apply &&apply) {
  return check_eigenpairs(
      nEv, opType, lambda_h, residual_h, sigma_h, [&](int v0, int n) { return apply(Y, ev + v0, n); },
      [&](int v0, int n, double *sums) { return coarse_scalars(0, ev + v0, Y, n, scal_d, comm, stream, sums); },
      [&](int v0, int n, const double *lambda, double *sums) -> int {
        MUGIQ_CHECK_HIP(hipMemcpyAsync(scal_d, lambda, sizeof(double) * 2 * n, hipMemcpyHostToDevice, stream));
        return coarse_scalars(1, ev + v0, Y, n, scal_d, comm, stream, sums);
      });
}

}  // namespace

int compute_evals_coarse(const MugiqHipCoarseField *ev, int nEv, const MugiqHipTransfer *transfers, int nLevels, const MugiqHipGaugeField *gauge,
                         const MugiqHipCloverField *clover, double kappa, int opType, int massNormalization, double *lambda_h, double *residual_h,
                         double *sigma_h, const MugiqHipComm *comm, hipStream_t stream) {
  const char *who = "computeEvalsCoarse";
  // ---- validation, before any device work
  MUGIQ_REQUIRE(ev != nullptr && transfers != nullptr && lambda_h != nullptr && residual_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nEv >= 1, "%s: nEv = %d must be >= 1", who, nEv);
  MUGIQ_REQUIRE(nLevels >= 1 && nLevels <= 8, "%s: nCoarseLevels = %d must be in [1, 8]", who, nLevels);
  int st, part[4];
  if ((st = check_evals_request(opType, sigma_h, massNormalization, kappa, who))) return st;
  std::vector<MugiqHipCoarseField> lev;
  if ((st = validate_hierarchy(transfers, nLevels, ev, nEv, &lev, who))) return st;
  const MugiqHipTransfer &T0 = transfers[0];
  if ((st = check_comm(comm, part, true, who))) return st;
  if ((st = check_gauge(gauge, T0.X, part, who))) return st;
  const TransferGeom g0 = transfer_geom(T0);
  if (clover) {
    if ((st = validate_clover(clover, T0.X, g0.volumeCB, who))) return st;
    MUGIQ_REQUIRE(clover->precision == gauge->precision, "%s: clover precision %d differs from the gauge precision %d", who, clover->precision, gauge->precision);
  }
  if ((st = debug_poison_lds_if_asked(stream))) return st;

  // ---- work memory (per-stream workspace): [the prolongator's packed coarse vectors][the send buffer of the stencil's halo exchange]
  // [2 x 8 fine vectors with ghost zones][2 x 8 coarse vectors on every level][lambda and sums]
  const size_t P = (size_t)T0.precision;
  const TransferSwitches sw = transfer_switches_from_env();
  MugiqHipSpinorField like{};  // a fine work vector, without a body
  like.precision = (int)P, like.field_order = 2, like.nParity = 2, like.volumeCB = like.stride = g0.volumeCB, like.parity_offset = (int64_t)12 * g0.volumeCB;
  for (int d = 0; d < 4; d++) like.X[d] = T0.X[d];
  const size_t packedBytes = align256(select_prolong_form(T0, T0.precision, like.field_order, kEvBlock, sw).workspaceBytes);
  const size_t sendBytes = align256(stencil_send_bytes(like, (int)P, part, kEvBlock));
  const size_t fineBody = align256((size_t)24 * g0.volumeCB * 2 * P);
  size_t zone[4], fineBytes = fineBody;
  for (int d = 0; d < 4; d++) {
    zone[d] = part[d] ? align256((size_t)24 * (g0.volumeCB / T0.X[d]) * 2 * P) : 0;
    fineBytes += 2 * zone[d];
  }
  std::vector<size_t> levBytes(nLevels);
  size_t bytes = packedBytes + sendBytes + 2 * kEvBlock * fineBytes;
  for (int l = 0; l < nLevels; l++) {
    levBytes[l] = align256((size_t)2 * lev[l].parity_offset * 2 * P);
    bytes += 2 * kEvBlock * levBytes[l];
  }
  const size_t scalOff = bytes;
  bytes += sizeof(double) * 5 * kEvBlock;
  void *ws = nullptr;
  if ((st = stream_workspace(&ws, bytes, stream))) return st;
  unsigned char *const packed = static_cast<unsigned char *>(ws), *cur = packed + packedBytes + sendBytes;
  const OpContext stencil{gauge, comm, {part[0], part[1], part[2], part[3]}, kappa, stream, packed + packedBytes, who, clover};
  MugiqHipSpinorField F[2][kEvBlock];
  for (int k = 0; k < 2; k++)
    for (int i = 0; i < kEvBlock; i++) {
      MugiqHipSpinorField f = like;
      f.data = cur;
      cur += fineBody;
      for (int d = 0; d < 4; d++)
        for (int b = 0; b < 2; b++) {
          f.ghost[d][b] = part[d] ? cur : nullptr;
          cur += zone[d];
        }
      F[k][i] = f;
    }
  // C[l][0]: the vectors in transit on level l + 1; on the coarsest level C[..][0] = A_c w and C[..][1] = the intermediate of a normal form
  std::vector<std::vector<MugiqHipCoarseField>> C(nLevels, std::vector<MugiqHipCoarseField>(2 * kEvBlock));
  for (int l = 0; l < nLevels; l++)
    for (int i = 0; i < 2 * kEvBlock; i++) {
      C[l][i] = lev[l];
      C[l][i].data = cur;
      cur += levBytes[l];
    }
  const int L = nLevels;
  const double scale = mass_scale(massNormalization, kappa);

  // out = s R [g5] M^(dag) P in: up through the levels, one batched stencil (its halo exchange included), down again.  The LDS is
  // poisoned (where asked) in front of every step up and of the stencil
  auto simple = [&](const MugiqHipCoarseField *out, const MugiqHipCoarseField *in, int n, int dagger, int gamma5, double s) -> int {
    int rc;
    const MugiqHipCoarseField *c = in;
    for (int l = L - 1; l >= 1; l--) {
      if ((rc = debug_poison_lds_if_asked(stream))) return rc;
      if ((rc = prolong_coarse_batched(C[l - 1].data(), c, n, &transfers[l], stream))) return rc;
      c = C[l - 1].data();
    }
    if ((rc = debug_poison_lds_if_asked(stream))) return rc;
    if ((rc = prolong_batched(F[0], c, n, &T0, sw, packed, stream))) return rc;
    if ((rc = debug_poison_lds_if_asked(stream))) return rc;
    if ((rc = stencil_apply(stencil, F[1], F[0], n, dagger, 0, s))) return rc;
    if ((rc = restrict_batched(L == 1 ? out : C[0].data(), F[1], n, &T0, gamma5, stream))) return rc;
    for (int l = 1; l < L; l++)
      if ((rc = restrict_coarse_batched(l == L - 1 ? out : C[l].data(), C[l - 1].data(), n, &transfers[l], stream))) return rc;
    return MUGIQ_HIP_SUCCESS;
  };
  // (QUDA's DiracMdagM / DiracMMdag on DiracCoarse: products of the coarse operators, not R MdagM P)
  const MugiqHipCoarseField *Tm = C[L - 1].data() + kEvBlock;
  return check_coarse_eigenpairs(ev, nEv, opType, C[L - 1].data(), reinterpret_cast<double *>(static_cast<unsigned char *>(ws) + scalOff), lambda_h,
                                 residual_h, sigma_h, comm, stream, [&](const MugiqHipCoarseField *y, const MugiqHipCoarseField *w, int n) {
                                   return apply_form(opType, simple, y, w, Tm, n, scale);
                                 });
}

// The same check with A_c applied by the explicit coarse operator (csrc/coarse_op.hip) instead of R M P through the fine lattice: one
// level, one domain (an unpartitioned comm of several ranks passes check_single_domain: every rank checks its own vectors, nothing is
// summed).  Work memory (operator workspace of the stream; coarse_apply keeps its intermediate in stream_workspace): 8 coarse vectors laid
// out like the eigenvectors, lambda and the sums
// grid: mugiq_hip_compute_evals_coarse_operator_grid -- A_c by coarse_apply_grid (the faces of every launch exchanged, the halo's matrices
// for M^dag), the sums added over the ranks in their fixed order
int compute_evals_coarse_operator(const MugiqHipCoarseField *ev, int nEv, const MugiqHipCoarseOperator *op, const MugiqHipCoarseHalo *halo, int opType,
                                  int massNormalization, double *lambda_h, double *residual_h, double *sigma_h, const MugiqHipComm *comm,
                                  hipStream_t stream, bool grid) {
  const char *who = grid ? "computeEvalsCoarseGrid" : "computeEvalsCoarse(coarseOp)";
  // ---- validation, before any device work
  MUGIQ_REQUIRE(ev != nullptr && lambda_h != nullptr && residual_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nEv >= 1, "%s: nEv = %d must be >= 1", who, nEv);
  int st, part[4] = {0, 0, 0, 0};
  if (grid) {
    if ((st = check_coarse_grid(comm, op, halo, part, true, who))) return st;
  } else {
    if ((st = check_single_domain(comm, who))) return st;
    if ((st = validate_coarse_operator(op, who))) return st;
  }
  if ((st = check_evals_request(opType, sigma_h, massNormalization, op->kappa, who))) return st;
  if ((st = validate_coarse_vectors(ev, nEv, op, who, "coarse eigen"))) return st;
  if ((st = debug_poison_lds_if_asked(stream))) return st;

  const size_t one = align256((size_t)2 * ev[0].parity_offset * 2 * (size_t)op->precision);
  void *ws = nullptr;
  if ((st = stream_operator_workspace(&ws, kEvBlock * one + sizeof(double) * 5 * kEvBlock, stream))) return st;
  MugiqHipCoarseField Y[kEvBlock];
  for (int i = 0; i < kEvBlock; i++) {
    Y[i] = ev[0];
    Y[i].data = static_cast<unsigned char *>(ws) + i * one;
  }
  const double scale = mass_scale(massNormalization, op->kappa);
  return check_coarse_eigenpairs(ev, nEv, opType, Y, reinterpret_cast<double *>(static_cast<unsigned char *>(ws) + kEvBlock * one), lambda_h, residual_h,
                                 sigma_h, grid ? comm : nullptr, stream, [&](const MugiqHipCoarseField *y, const MugiqHipCoarseField *w, int n) {
                                   return coarse_apply_grid(y, w, n, op, halo, part, opType, scale, comm, stream);  // (one domain: coarse_apply)
                                 });
}

}  // namespace mugiq

using namespace mugiq;

extern "C" {

int mugiq_hip_restrict_batched(const MugiqHipCoarseField *coarse_h, const MugiqHipSpinorField *fine_h, int nVec, const MugiqHipTransfer *transfer,
                               int gamma5, void *stream) {
  if (int st = validate_restrict(coarse_h, fine_h, nVec, transfer, "restrictVecs")) return st;
  if (int dbg_ = debug_poison_lds_if_asked(static_cast<hipStream_t>(stream))) return dbg_;
  return restrict_batched(coarse_h, fine_h, nVec, transfer, gamma5, static_cast<hipStream_t>(stream));
}

int mugiq_hip_restrict_coarse_batched(const MugiqHipCoarseField *coarser_h, const MugiqHipCoarseField *finer_h, int nVec,
                                      const MugiqHipTransfer *transfer, void *stream) {
  if (int st = validate_coarse_transfer(transfer, finer_h, coarser_h, nVec, "restrictVecs(coarse level)")) return st;
  if (int dbg_ = debug_poison_lds_if_asked(static_cast<hipStream_t>(stream))) return dbg_;
  return restrict_coarse_batched(coarser_h, finer_h, nVec, transfer, static_cast<hipStream_t>(stream));
}

int mugiq_hip_deflate_low_modes_coarse(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec,
                                       const MugiqHipCoarseField *coarseEvecs_h, const double *sigma_h, int nEv,
                                       const MugiqHipTransfer *transfers_h, int nCoarseLevels, int gamma5, double *overlaps_h,
                                       const MugiqHipComm *comm, void *stream) {
  return deflate_low_modes_coarse(dst_h, src_h, nVec, coarseEvecs_h, sigma_h, nEv, transfers_h, nCoarseLevels, gamma5, overlaps_h, comm,
                                  static_cast<hipStream_t>(stream), "deflateLowModesCoarse");
}

int mugiq_hip_compute_evals_coarse(const MugiqHipCoarseField *coarseEvecs_h, int nEv, const MugiqHipTransfer *transfers_h, int nCoarseLevels,
                                   const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover, double kappa, int opType,
                                   int massNormalization, double *lambda_h, double *residual_h, double *sigma_h, const MugiqHipComm *comm,
                                   void *stream) {
  return compute_evals_coarse(coarseEvecs_h, nEv, transfers_h, nCoarseLevels, gauge, clover, kappa, opType, massNormalization, lambda_h, residual_h,
                              sigma_h, comm, static_cast<hipStream_t>(stream));
}

int mugiq_hip_compute_evals_coarse_operator(const MugiqHipCoarseField *coarseEvecs_h, int nEv, const MugiqHipCoarseOperator *op, int opType,
                                            int massNormalization, double *lambda_h, double *residual_h, double *sigma_h,
                                            const MugiqHipComm *comm, void *stream) {
  return compute_evals_coarse_operator(coarseEvecs_h, nEv, op, nullptr, opType, massNormalization, lambda_h, residual_h, sigma_h, comm,
                                       static_cast<hipStream_t>(stream), false);
}

int mugiq_hip_compute_evals_coarse_operator_grid(const MugiqHipCoarseField *coarseEvecs_h, int nEv, const MugiqHipCoarseOperator *op,
                                                 const MugiqHipCoarseHalo *halo, int opType, int massNormalization, double *lambda_h,
                                                 double *residual_h, double *sigma_h, const MugiqHipComm *comm, void *stream) {
  return compute_evals_coarse_operator(coarseEvecs_h, nEv, op, halo, opType, massNormalization, lambda_h, residual_h, sigma_h, comm,
                                       static_cast<hipStream_t>(stream), true);
}

}  // extern "C"
