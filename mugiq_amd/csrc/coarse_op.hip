// The Galerkin coarse operator M_c = R M P of a finest-level transfer as an explicit stencil (QUDA's DiracCoarse, which the reference's
// computeCoarse branch works on: lib/eigsolve_mugiq.cpp:27-33): nine dense N x N matrices per coarse site, N = 2 n_vec, built once per
// configuration from V, the links and the clover term, and applied on the coarse grid without touching a fine vector.  Definitions, storage
// and limits: MugiqHipCoarseOperator in include/mugiq_hip.h.
//
// Numerics (csrc/mg_common.h): products and sums in fp64 whatever the storage, one rounding on the store, no atomics, and a
// summation order fixed by the shape of the transfer (build) or by N (apply) alone.
//
// coarse_build_kernel: a workgroup owns one matrix m of one aggregate X (and, for N^2 > 4096, one chunk of 4096 of its elements); lane t
// carries the elements t, t + 256, ... in registers.  It walks the sites x of the aggregate in lexicographic order and, per site, the
// terms that belong to the matrix (Xd: the site term, then the hops that stay inside; Y: the one hop that leaves).  Per term the
// workgroup stages V(x) (12 x n_vec, once per site) and W = K V(x') (12 x N: the link, the spin projector and -kappa -- or the clover
// blocks -- applied to the neighbour's rows; 1 -+ g_mu couples a spin to itself and to ONE spin of the other chirality) in LDS as fp64,
// then every lane adds the six products conj(V(x; s c, j)) W(s c; S' j') of its elements.  6 N^2 complex products per term against
// 36 N for W: the vector pipe, from LDS.  Once per configuration; measured in DESIGN.md 4.4b.
//
// coarse_apply_kernel: a workgroup owns one coarse site, a block of 8 vectors and 64 output components.  The nine matrices are streamed
// from global memory exactly once per block of 8 (rows of 16 consecutive elements per 16-lane group: 256-byte runs), the eight input
// vectors of the neighbour wait in LDS as fp64.  M: lane (g, l) adds the columns l, l + 16, ... of its rows g + 16 i; M^dag (the explicit
// adjoint: the matrices of the neighbour sites, conjugate-transposed) reads the same runs and adds the rows g, g + 16, ... into its
// columns l + 16 k.  The 16 partial sums of an output meet in LDS and are added in a fixed order by one lane.  Every vector has its own
// accumulators and the same order wherever it stands in the batch.
#include "mg_common.h"
#include "op_forms.h"

#include <algorithm>
#include <vector>

namespace mugiq {
namespace {

constexpr int kCbThreads = 256;  // build: lanes of a workgroup
constexpr int kCbEPT = 16;       // ... matrix elements a lane carries
constexpr int kCaThreads = 256;  // apply: 16 groups x 16 lanes
constexpr int kCaRB = 8;         // ... vectors per workgroup
constexpr int kCaOut = 64;       // ... output components per workgroup (4 per group or lane); the small-lattice forms take 32 or 16

static_assert(kGammaColumn[15][0] == 0 && kGammaColumn[15][3] == 3 && kGammaPhase[15][0] == 0 && kGammaPhase[15][1] == 0 && kGammaPhase[15][2] == 2 &&
                  kGammaPhase[15][3] == 2, "g5 = diag(1, 1, -1, -1): G5 of the coarse operator is +1 on chirality 0 and -1 on chirality 1");

// i^ph * z
__device__ inline Cplx<double> mul_phase(int ph, const Cplx<double> &z) {
  switch (ph & 3) {
  case 0: return z;
  case 1: return Cplx<double>{-z.im, z.re};
  case 2: return Cplx<double>{-z.re, -z.im};
  default: return Cplx<double>{z.im, -z.re};
  }
}
// row s of g_mu = Gamma_G: (g psi)_s = i^ph psi_col
template <int G> __device__ inline void gamma_row(int s, int *ph, int *col) {
  static_assert(kGammaColumn[G][0] >= 2 && kGammaColumn[G][1] >= 2 && kGammaColumn[G][2] < 2 && kGammaColumn[G][3] < 2, "g_mu must flip the chirality");
  *ph = s == 0 ? kGammaPhase[G][0] : s == 1 ? kGammaPhase[G][1] : s == 2 ? kGammaPhase[G][2] : kGammaPhase[G][3];
  *col = s == 0 ? kGammaColumn[G][0] : s == 1 ? kGammaColumn[G][1] : s == 2 ? kGammaColumn[G][2] : kGammaColumn[G][3];
}
__device__ inline void gamma_mu_row(int mu, int s, int *ph, int *col) {
  switch (mu) {  // g_x, g_y, g_z, g_t = Gamma_1, Gamma_2, Gamma_4, Gamma_8 (csrc/wilson.hip)
  case 0: gamma_row<1>(s, ph, col); break;
  case 1: gamma_row<2>(s, ph, col); break;
  case 2: gamma_row<4>(s, ph, col); break;
  default: gamma_row<8>(s, ph, col); break;
  }
}

// ---- the build ----------------------------------------------------------------------------------------------------------------------
struct CoarseBuildArgs {
  const void *V;  // [parity][(3s+c)*NV + j][x_cb]
  int64_t Vpo;
  int Vstride, NV;
  TransferGeom g;
  const void *U;  // border-extended links, addressed as by the stencil (csrc/wilson.hip)
  int XE[4], brd[4], gstride;
  int64_t gpo;
  const void *A;  // packed clover blocks (NULL: A = 1)
  int Astride;
  int64_t Apo;
  void *out;
  double kappa;
};

template <typename FV, typename FG> __global__ __launch_bounds__(kCbThreads) void coarse_build_kernel(CoarseBuildArgs a) {
  extern __shared__ Cplx<double> build_lds[];
  __shared__ Cplx<double> Um[9], Acl[72];
  const int NV = a.NV, N = 2 * NV, t = threadIdx.x;
  Cplx<double> *Vx = build_lds, *W = build_lds + 12 * NV;  // V(x): [12][NV];  W: [12][N]
  const int site = blockIdx.x, m = blockIdx.y;
  const int cpar = site / a.g.volumeCBc, xc_cb = site - cpar * a.g.volumeCBc;
  int cc[4];
  get_coords(cc, xc_cb, a.g.Xc, cpar);

  // the elements of this lane: e = r N + c, r = S NV + j
  const int e0 = blockIdx.z * (kCbThreads * kCbEPT) + t;
  int vOff[kCbEPT], wOff[kCbEPT];
  Cplx<double> acc[kCbEPT];
#pragma unroll
  for (int i = 0; i < kCbEPT; i++) {
    const int e = min(e0 + kCbThreads * i, N * N - 1);  // (lanes past the end shadow the last element; they do not store)
    const int r = e / N, c = e - r * N, S = r / NV, j = r - S * NV;
    vOff[i] = S * 6 * NV + j;
    wOff[i] = S * 6 * N + c;
    acc[i] = Cplx<double>{0.0, 0.0};
  }

  for (int k = 0; k < a.g.aggVol; k++) {
    int loc[4], x[4], q = k;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      loc[d] = q % a.g.bs[d];
      q /= a.g.bs[d];
      x[d] = cc[d] * a.g.bs[d] + loc[d];
    }
    const int pty = (x[0] + x[1] + x[2] + x[3]) & 1, x_cb = lex_index(x, a.g.X) >> 1;
    bool staged = false;  // V(x) is in LDS
    // term 0: the site term A(x); term 1 + 2 mu: the hop to x + mu; term 2 + 2 mu: the hop to x - mu.  Xd takes the site term and the
    // hops that stay inside the aggregate, Y+-_mu the one hop that leaves it (every condition is uniform over the workgroup)
    for (int term = (m == 0 ? 0 : m); term <= (m == 0 ? 8 : m); term++) {
      const int mu = (term - 1) >> 1, fwd = term & 1;
      if (term > 0) {
        const bool inside = fwd ? loc[mu] + 1 < a.g.bs[mu] : loc[mu] >= 1;
        if (inside != (m == 0)) continue;
      }
      __syncthreads();  // the products of the previous term have been taken
      if (!staged) {
        for (int i = t; i < 12 * NV; i += kCbThreads) Vx[i] = ld_wide<FV>(a.V, pty * a.Vpo + (int64_t)i * a.Vstride + x_cb);
        staged = true;
      }
      if (term == 0) {
        if (a.A != nullptr && t < 72) {  // the two Hermitian 6 x 6 blocks, dense (packing: MugiqHipCloverField)
          const int b = t / 36, i = (t - 36 * b) / 6, j = t - 36 * b - 6 * i;
          const int64_t base = pty * a.Apo + x_cb;
          Cplx<double> v;
          if (i == j) {
            const Cplx<double> d = ld_wide<FG>(a.A, base + (int64_t)(18 * b + (i >> 1)) * a.Astride);
            v = Cplx<double>{(i & 1) ? d.im : d.re, 0.0};
          } else {
            const int hi = max(i, j), lo = min(i, j);
            v = ld_wide<FG>(a.A, base + (int64_t)(18 * b + 3 + hi * (hi - 1) / 2 + lo) * a.Astride);
            if (i < j) v.im = -v.im;
          }
          Acl[t] = v;
        }
      } else if (t < 9) {  // U_mu(x) | U_mu^dag(x - mu): the conjugate transpose of the stored link
        int c2[4], dx1[4] = {0, 0, 0, 0};
#pragma unroll
        for (int d = 0; d < 4; d++) c2[d] = x[d] + a.brd[d];
        if (!fwd) dx1[mu] = -1;
        const int lidx = link_index_shift(c2, dx1, a.XE), lpty = fwd ? pty : 1 - pty;
        const int row = t / 3, col = t - 3 * row;
        const int el = fwd ? row * 3 + col : col * 3 + row;
        Cplx<double> u = ld_wide<FG>(a.U, lpty * a.gpo + (int64_t)(mu * 9 + el) * a.gstride + lidx);
        if (!fwd) u.im = -u.im;
        Um[t] = u;
      }
      __syncthreads();
      if (term == 0) {
        for (int idx = t; idx < 12 * N; idx += kCbThreads) {
          const int row = idx / N, col = idx - row * N, Sp = col / NV, jp = col - Sp * NV, b = row / 6;
          Cplx<double> w{0.0, 0.0};
          if (b == Sp) {  // A is block diagonal in the chirality
            if (a.A == nullptr) w = Vx[row * NV + jp];
            else
              for (int ip = 0; ip < 6; ip++) cmadd(w, Acl[b * 36 + (row - 6 * b) * 6 + ip], Vx[(6 * b + ip) * NV + jp]);
          }
          W[idx] = w;
        }
      } else {
        int dx[4] = {0, 0, 0, 0};
        dx[mu] = fwd ? 1 : -1;
        const int npty = 1 - pty, nidx = link_index_shift(x, dx, a.g.X);
        const double sg = fwd ? -1.0 : 1.0;  // (1 - g_mu) forward, (1 + g_mu) backward
        for (int idx = t; idx < 8 * NV; idx += kCbThreads) {
          const int s = idx / N, rem = idx - s * N, Sp = rem / NV, jp = rem - Sp * NV;
          int ph, col;
          gamma_mu_row(mu, s, &ph, &col);
          const bool same = (s >> 1) == Sp;
          const int ss = same ? s : col;  // the spin of chirality Sp that (1 -+ g_mu) couples s to
          Cplx<double> T[3];
#pragma unroll
          for (int cp = 0; cp < 3; cp++) {
            const Cplx<double> v = ld_wide<FV>(a.V, npty * a.Vpo + (int64_t)((3 * ss + cp) * NV + jp) * a.Vstride + nidx);
            const Cplx<double> gv = mul_phase(ph, v);
            T[cp] = same ? v : Cplx<double>{sg * gv.re, sg * gv.im};
          }
#pragma unroll
          for (int c = 0; c < 3; c++) {
            Cplx<double> w{0.0, 0.0};
#pragma unroll
            for (int cp = 0; cp < 3; cp++) cmadd(w, Um[c * 3 + cp], T[cp]);
            W[(3 * s + c) * N + rem] = Cplx<double>{-a.kappa * w.re, -a.kappa * w.im};
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kCbEPT; i++)
#pragma unroll
        for (int sc = 0; sc < 6; sc++) cmadd_conj(acc[i], Vx[vOff[i] + sc * NV], W[wOff[i] + sc * N]);
    }
  }
  const int64_t obase = ((int64_t)site * 9 + m) * N * N;
#pragma unroll
  for (int i = 0; i < kCbEPT; i++) {
    const int e = e0 + kCbThreads * i;
    if (e < N * N) st_round<FV>(a.out, obase + e, acc[i]);
  }
}

template <typename FV, typename FG>
int launch_build(const MugiqHipCoarseOperator *op, const MugiqHipTransfer *T, const MugiqHipGaugeField *U, const MugiqHipCloverField *C, double kappa,
                 hipStream_t stream) {
  CoarseBuildArgs a;
  a.V = T->V;
  a.Vpo = T->parity_offset;
  a.Vstride = T->stride;
  a.NV = T->nVec;
  a.g = transfer_geom(*T);
  a.U = U->data;
  for (int d = 0; d < 4; d++) {
    a.brd[d] = U->R[d];
    a.XE[d] = T->X[d] + 2 * U->R[d];
  }
  a.gstride = U->stride;
  a.gpo = U->parity_offset;
  a.A = C ? C->data : nullptr;
  a.Astride = C ? C->stride : 0;
  a.Apo = C ? C->parity_offset : 0;
  a.out = op->data;
  a.kappa = kappa;
  const int N = 2 * a.NV, per = kCbThreads * kCbEPT;
  const dim3 grid(2 * a.g.volumeCBc, 9, (N * N + per - 1) / per);
  const size_t lds = sizeof(Cplx<double>) * (size_t)(12 * a.NV + 12 * N);
  hipLaunchKernelGGL((coarse_build_kernel<FV, FG>), grid, dim3(kCbThreads), lds, stream, a);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

// ---- the application ----------------------------------------------------------------------------------------------------------------
struct CoarseApplyArgs {
  const void *op;
  int NV, Xc[4], volumeCBc;
  const void *const *tab;  // device table: nVec src bodies, then nVec dst bodies
  int Sstride, Dstride;
  int64_t Spo, Dpo;
  int nVec, gamma5;
  double scale;
};

// OUT = 64 | 32 | 16 output components per workgroup: every 16-lane group (M) or lane (M^dag) owns OUT / 16 of them, and blockIdx.z walks
// N / OUT chunks.  What one output is made of does not depend on OUT -- the 9 matrices in order, lane l over c = l, l + 16, ..., then
// the 16 partial sums in ascending order, every product an explicit fma -- so all three give the same bits; a smaller OUT only spreads a
// small lattice over more workgroups (launch_apply chooses)
template <typename F, int DAG, int OUT> __global__ __launch_bounds__(kCaThreads) void coarse_apply_kernel(CoarseApplyArgs a) {
  static_assert(OUT == 16 || OUT == 32 || OUT == 64, "outputs per workgroup");
  constexpr int NI = OUT / 16;                     // outputs per group or lane
  extern __shared__ Cplx<double> in_s[];           // [8][N]: the input vectors at the neighbour of the current matrix
  __shared__ Cplx<double> red[16][kCaRB][16 + 1];  // the 16 partial sums of 16 outputs x 8 vectors
  const int NV = a.NV, N = 2 * NV, t = threadIdx.x, l = t & 15, g = t >> 4;
  const int site = blockIdx.x, n0 = blockIdx.y * kCaRB, o0 = blockIdx.z * OUT;
  const int cpar = site / a.volumeCBc, xc_cb = site - cpar * a.volumeCBc;
  int cc[4];
  get_coords(cc, xc_cb, a.Xc, cpar);
  const auto *tab = as_constant(a.tab);
  Cplx<double> acc[NI][kCaRB];
#pragma unroll
  for (int i = 0; i < NI; i++)
#pragma unroll
    for (int v = 0; v < kCaRB; v++) acc[i][v] = Cplx<double>{0.0, 0.0};

  for (int m = 0; m < 9; m++) {
    // the input site: X (m = 0), X + mu (m = 1 + 2 mu), X - mu (m = 2 + 2 mu);  M: matrix m of X;  M^dag: the matrix of the input site that hops
    // back to X, Y-_mu(X + mu)^dag | Y+_mu(X - mu)^dag
    const int mu = (m - 1) >> 1, fwd = m & 1;
    int nc[4] = {cc[0], cc[1], cc[2], cc[3]};
    if (m > 0) nc[mu] = (cc[mu] + (fwd ? 1 : a.Xc[mu] - 1)) % a.Xc[mu];
    const int npar = m == 0 ? cpar : 1 - cpar, nx = lex_index(nc, a.Xc) >> 1;
    const int msite = DAG ? npar * a.volumeCBc + nx : site, mm = (DAG && m > 0) ? (fwd ? m + 1 : m - 1) : m;
    const int64_t mbase = ((int64_t)msite * 9 + mm) * N * N;
    __syncthreads();  // the previous matrix is through
    for (int idx = t; idx < kCaRB * N; idx += kCaThreads) {
      const int v = idx / N, c = idx - v * N;
      in_s[idx] = ld_wide<F>(tab[min(n0 + v, a.nVec - 1)], npar * a.Spo + (int64_t)c * a.Sstride + nx);  // (vectors past the end shadow the last one)
    }
    __syncthreads();
    if constexpr (!DAG) {
      for (int c = l; c < N; c += 16) {
        Cplx<double> x[kCaRB];
#pragma unroll
        for (int v = 0; v < kCaRB; v++) x[v] = in_s[v * N + c];
#pragma unroll
        for (int i = 0; i < NI; i++) {
          const int r = o0 + g + 16 * i;
          if (r < N) {
            const Cplx<double> e = ld_wide<F>(a.op, mbase + (int64_t)r * N + c);
#pragma unroll
            for (int v = 0; v < kCaRB; v++) cmadd(acc[i][v], e, x[v]);
          }
        }
      }
    } else {
      for (int r = g; r < N; r += 16) {
        Cplx<double> x[kCaRB];
#pragma unroll
        for (int v = 0; v < kCaRB; v++) x[v] = in_s[v * N + r];
#pragma unroll
        for (int k = 0; k < NI; k++) {
          const int c = o0 + l + 16 * k;
          if (c < N) {
            const Cplx<double> e = ld_wide<F>(a.op, mbase + (int64_t)r * N + c);
#pragma unroll
            for (int v = 0; v < kCaRB; v++) cmadd_conj(acc[k][v], e, x[v]);
          }
        }
      }
    }
  }
  // output o0 + p + 16 i, p = g (M) | l (M^dag): its 16 partial sums, added in ascending order by one lane
#pragma unroll
  for (int i = 0; i < NI; i++) {
    __syncthreads();  // the previous trip has been read
#pragma unroll
    for (int v = 0; v < kCaRB; v++) red[DAG ? l : g][v][DAG ? g : l] = acc[i][v];
    __syncthreads();
    if (t < 16 * kCaRB) {
      const int p = t / kCaRB, v = t - p * kCaRB, o = o0 + p + 16 * i;
      Cplx<double> s{0.0, 0.0};
      for (int q = 0; q < 16; q++) {
        s.re += red[p][v][q].re;
        s.im += red[p][v][q].im;
      }
      if (o < N && n0 + v < a.nVec) {
        const double f = (a.gamma5 && o >= NV) ? -a.scale : a.scale;  // G5 = diag(g5(S))
        st_round<F>(const_cast<void *>(tab[a.nVec + n0 + v]), cpar * a.Dpo + (int64_t)o * a.Dstride + xc_cb, Cplx<double>{f * s.re, f * s.im});
      }
    }
  }
}

// The outputs per workgroup of coarse_apply_kernel for one launch on n vectors, decided here and nowhere else, on the host: from the
// workgroups the 64-output grid would have, 2 volumeCB sites x ceil(n / 8) blocks of vectors x ceil(N / 64) chunks.  With one workgroup per
// coarse site (256 at 4^4 with N = 64, one per compute unit) the 64-output form leaves the device short of waves; the 32-output form, twice
// as many workgroups that each read the same inputs and half of the matrix rows, took 0.69 x its time there and 1.18 x at 512 workgroups
// (the 16-output form: 0.83 x and 1.26 x).  MUGIQ_HIP_COARSE_APPLY_OUT = 16 | 32 | 64 overrides the rule (anything else is
// ignored); the bits do not depend on it.  launch_apply and the host query mugiq_hip_coarse_apply_outputs both ask here
constexpr int64_t kCaSmallGrid = 512;
dim3 apply_grid64(const MugiqHipCoarseOperator *op, int n) {
  return dim3(2 * op->volumeCB, (n + kCaRB - 1) / kCaRB, (2 * op->nVec + kCaOut - 1) / kCaOut);
}
int apply_outputs_per_workgroup(const MugiqHipCoarseOperator *op, int n) {
  if (const char *e = getenv("MUGIQ_HIP_COARSE_APPLY_OUT")) {
    const int o = atoi(e);
    if (o == 16 || o == 32 || o == 64) return o;
  }
  const dim3 g = apply_grid64(op, n);
  return (int64_t)g.x * g.y * g.z < kCaSmallGrid ? 32 : kCaOut;
}

template <typename F, int DAG>
void launch_apply_form(int out, dim3 grid, size_t lds, hipStream_t stream, const CoarseApplyArgs &a, int N) {
  grid.z = (N + out - 1) / out;
  if (out == 16) hipLaunchKernelGGL((coarse_apply_kernel<F, DAG, 16>), grid, dim3(kCaThreads), lds, stream, a);
  else if (out == 32) hipLaunchKernelGGL((coarse_apply_kernel<F, DAG, 32>), grid, dim3(kCaThreads), lds, stream, a);
  else hipLaunchKernelGGL((coarse_apply_kernel<F, DAG, 64>), grid, dim3(kCaThreads), lds, stream, a);
}

// dst_i = scale [G5] M_c^(dag) src_i, i < n
int launch_apply(const MugiqHipCoarseField *dst, const MugiqHipCoarseField *src, int n, const MugiqHipCoarseOperator *op, int dagger, int gamma5,
                 double scale, hipStream_t stream) {
  std::vector<const void *> host(2 * (size_t)n);
  for (int i = 0; i < n; i++) {
    host[i] = src[i].data;
    host[n + i] = dst[i].data;
  }
  void *dev = nullptr;
  if (int st = upload_table(&dev, host.data(), host.size() * sizeof(void *), stream)) return st;
  CoarseApplyArgs a;
  a.op = op->data;
  a.NV = op->nVec;
  for (int d = 0; d < 4; d++) a.Xc[d] = op->X[d];
  a.volumeCBc = op->volumeCB;
  a.tab = static_cast<const void *const *>(dev);
  a.Sstride = src[0].stride;
  a.Spo = src[0].parity_offset;
  a.Dstride = dst[0].stride;
  a.Dpo = dst[0].parity_offset;
  a.nVec = n;
  a.gamma5 = gamma5 ? 1 : 0;
  a.scale = scale;
  const int N = 2 * op->nVec;
  const dim3 grid = apply_grid64(op, n);
  const int out = apply_outputs_per_workgroup(op, n);
  const size_t lds = sizeof(Cplx<double>) * (size_t)kCaRB * N;
  if (op->precision == 8 && !dagger) launch_apply_form<double, 0>(out, grid, lds, stream, a, N);
  else if (op->precision == 8) launch_apply_form<double, 1>(out, grid, lds, stream, a, N);
  else if (!dagger) launch_apply_form<float, 0>(out, grid, lds, stream, a, N);
  else launch_apply_form<float, 1>(out, grid, lds, stream, a, N);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

size_t operator_elems(const int Xc[4], int nVec) {
  size_t vol = 1;
  for (int d = 0; d < 4; d++) vol *= (size_t)Xc[d];
  return vol * 9 * (size_t)(2 * nVec) * (size_t)(2 * nVec);
}

}  // namespace

int check_single_domain(const MugiqHipComm *comm, const char *who) {
  if (comm == nullptr) return MUGIQ_HIP_SUCCESS;
  bool part = comm->size > 1;
  for (int d = 0; d < 4; d++) part |= comm_partitioned(comm, d);
  if (part)
    return set_error(MUGIQ_HIP_ERROR_UNSUPPORTED,
                     "%s: the explicit coarse operator is built and applied on a single domain only (comm size %d, or a partitioned axis); "
                     "mugiq_hip_compute_evals_coarse serves process grids",
                     who, comm->size);
  return MUGIQ_HIP_SUCCESS;
}

int validate_coarse_operator(const MugiqHipCoarseOperator *op, const char *who) {
  MUGIQ_REQUIRE(op != nullptr && op->data != nullptr, "%s: coarse operator is NULL", who);
  MUGIQ_REQUIRE(op->precision == 4 || op->precision == 8, "%s: coarse operator precision %d", who, op->precision);
  MUGIQ_REQUIRE(op->nVec >= 1 && op->nVec <= kTransferMaxNV, "%s: coarse operator n_vec = %d must be in [1, %d]", who, op->nVec, kTransferMaxNV);
  long long vol = 1;
  for (int d = 0; d < 4; d++) {
    MUGIQ_REQUIRE(op->X[d] > 0 && (op->X[d] & 1) == 0, "%s: coarse operator X[%d] = %d must be positive and even", who, d, op->X[d]);
    vol *= op->X[d];
  }
  MUGIQ_REQUIRE(vol / 2 < (1LL << 30) && op->volumeCB == (int)(vol / 2), "%s: coarse operator volumeCB = %d, its dims give %lld", who, op->volumeCB, vol / 2);
  return MUGIQ_HIP_SUCCESS;
}

int validate_transfer_operator(const MugiqHipTransfer *T, const MugiqHipCoarseOperator *op, const char *who) {
  for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(T->X[d] > 0 && T->geoBlockSize[d] >= 1, "%s: transfer X / geo_block_size[%d]", who, d);
  MugiqHipCoarseField c0 = coarse_side_layout(*T);
  c0.data = reinterpret_cast<void *>(uintptr_t(16));  // geometry only: never read
  if (int st = validate_transfer(T, &c0, who)) return st;  // a finest-level transfer (spin_block_size 2), even coarse dims
  MUGIQ_REQUIRE(op->precision == T->precision, "%s: the coarse operator has precision %d, the transfer %d", who, op->precision, T->precision);
  MUGIQ_REQUIRE(op->nVec == T->nVec, "%s: the coarse operator has n_vec %d, the transfer %d", who, op->nVec, T->nVec);
  for (int d = 0; d < 4; d++)
    MUGIQ_REQUIRE(op->X[d] == c0.X[d], "%s: coarse operator X[%d] = %d, the transfer's coarse lattice has %d", who, d, op->X[d], c0.X[d]);
  return MUGIQ_HIP_SUCCESS;
}

int validate_coarse_vectors(const MugiqHipCoarseField *f, int n, const MugiqHipCoarseOperator *op, const char *who, const char *name) {
  for (int i = 0; i < n; i++) {
    const MugiqHipCoarseField &w = f[i];
    MUGIQ_REQUIRE(w.data != nullptr, "%s: %s vector %d is NULL", who, name, i);
    MUGIQ_REQUIRE(w.precision == op->precision, "%s: %s vector %d has precision %d, the coarse operator %d", who, name, i, w.precision, op->precision);
    MUGIQ_REQUIRE(w.nSpin == 2 && w.nColor == op->nVec, "%s: %s vector %d has nSpin %d, nColor %d; the coarse operator acts on nSpin 2, nColor %d", who, name, i,
                  w.nSpin, w.nColor, op->nVec);
    for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(w.X[d] == op->X[d], "%s: %s vector %d: X[%d] = %d, the coarse operator's is %d", who, name, i, d, w.X[d], op->X[d]);
    MUGIQ_REQUIRE(w.volumeCB == op->volumeCB && w.stride >= w.volumeCB && w.parity_offset >= (int64_t)2 * w.nColor * w.stride && w.stride == f[0].stride &&
                      w.parity_offset == f[0].parity_offset,
                  "%s: %s vector %d: volumeCB / stride / parity_offset", who, name, i);
  }
  return MUGIQ_HIP_SUCCESS;
}

// validated arguments; the intermediate of a normal form: 8 unpadded vectors in the per-stream workspace
int coarse_apply(const MugiqHipCoarseField *dst, const MugiqHipCoarseField *src, int nVec, const MugiqHipCoarseOperator *op, int opType, double scale,
                 hipStream_t stream) {
  auto simple = [&](const MugiqHipCoarseField *d, const MugiqHipCoarseField *s, int n, int dagger, int gamma5, double f) {
    return launch_apply(d, s, n, op, dagger, gamma5, f, stream);
  };
  MugiqHipCoarseField tmp[kCaRB];
  if (!normal_op(opType)) return apply_form(opType, simple, dst, src, tmp, nVec, scale);  // (one launch sequence for all nVec, no intermediate)
  const size_t one = align256((size_t)2 * 2 * op->nVec * op->volumeCB * 2 * op->precision);
  void *ws = nullptr;
  if (int st = stream_workspace(&ws, kCaRB * one, stream)) return st;
  for (int i = 0; i < kCaRB; i++) {
    tmp[i] = src[0];
    tmp[i].data = static_cast<unsigned char *>(ws) + i * one;
    tmp[i].stride = op->volumeCB;
    tmp[i].parity_offset = (int64_t)2 * op->nVec * op->volumeCB;
  }
  for (int v0 = 0; v0 < nVec; v0 += kCaRB)
    if (int st = apply_form(opType, simple, dst + v0, src + v0, tmp, std::min(kCaRB, nVec - v0), scale)) return st;
  return MUGIQ_HIP_SUCCESS;
}

}  // namespace mugiq

using namespace mugiq;

extern "C" {

size_t mugiq_hip_coarse_operator_bytes(const int X[4], int nVec, int precision) {
  if (!X || nVec < 1 || (precision != 4 && precision != 8)) return 0;
  return operator_elems(X, nVec) * 2 * (size_t)precision;
}

int mugiq_hip_alloc_coarse_operator(MugiqHipCoarseOperator *op, const int X[4], int nVec, int precision) {
  const char *who = "allocCoarseOperator";
  MUGIQ_REQUIRE(op && X, "%s: NULL argument", who);
  MUGIQ_REQUIRE(precision == 4 || precision == 8, "%s: precision %d", who, precision);
  MUGIQ_REQUIRE(nVec >= 1 && nVec <= kTransferMaxNV, "%s: n_vec = %d must be in [1, %d]", who, nVec, kTransferMaxNV);
  long long vol = 1;
  for (int d = 0; d < 4; d++) {
    MUGIQ_REQUIRE(X[d] > 0 && (X[d] & 1) == 0, "%s: X[%d] = %d must be positive and even", who, d, X[d]);
    op->X[d] = X[d];
    vol *= X[d];
  }
  MUGIQ_REQUIRE(vol / 2 < (1LL << 30), "%s: volume overflows int", who);
  op->precision = precision;
  op->nVec = nVec;
  op->volumeCB = (int)(vol / 2);
  op->kappa = 0.0;
  op->hasClover = 0;
  op->data = nullptr;
  const size_t bytes = mugiq_hip_coarse_operator_bytes(X, nVec, precision);
  MUGIQ_CHECK_HIP(hipMalloc(&op->data, bytes));
  MUGIQ_CHECK_HIP(hipMemset(op->data, 0, bytes));
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_free_coarse_operator(MugiqHipCoarseOperator *op) {
  if (op && op->data) {
    MUGIQ_CHECK_HIP(hipFree(op->data));
    op->data = nullptr;
  }
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_compute_coarse_operator(MugiqHipCoarseOperator *op, const MugiqHipTransfer *transfer, const MugiqHipGaugeField *gauge,
                                      const MugiqHipCloverField *clover, double kappa, const MugiqHipComm *comm, void *stream) {
  const char *who = "computeCoarseOperator";
  // ---- validation, before any device work
  MUGIQ_REQUIRE(op != nullptr && transfer != nullptr, "%s: NULL argument", who);
  int st;
  if ((st = check_single_domain(comm, who))) return st;
  if ((st = validate_coarse_operator(op, who))) return st;
  MUGIQ_REQUIRE(transfer->V != nullptr, "%s: transfer / null vectors are NULL", who);
  if ((st = validate_transfer_operator(transfer, op, who))) return st;
  const int part[4] = {0, 0, 0, 0};
  if ((st = check_gauge(gauge, transfer->X, part, who))) return st;
  const TransferGeom g = transfer_geom(*transfer);
  if (clover) {
    if ((st = validate_clover(clover, transfer->X, g.volumeCB, who))) return st;
    MUGIQ_REQUIRE(clover->precision == gauge->precision, "%s: clover precision %d differs from the gauge precision %d", who, clover->precision, gauge->precision);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  st = with_storage(transfer->precision, gauge->precision, [&](auto fv, auto fg) {
    return launch_build<decltype(fv), decltype(fg)>(op, transfer, gauge, clover, kappa, s);
  });
  if (st) return st;
  op->kappa = kappa;
  op->hasClover = clover ? 1 : 0;
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_coarse_apply(const MugiqHipCoarseField *dst_h, const MugiqHipCoarseField *src_h, int nVec, const MugiqHipCoarseOperator *op, int opType,
                           double scale, const MugiqHipComm *comm, void *stream) {
  const char *who = "coarseApply";
  MUGIQ_REQUIRE(dst_h != nullptr && src_h != nullptr && nVec >= 1, "%s: NULL / empty argument", who);
  int st;
  if ((st = check_single_domain(comm, who))) return st;
  if ((st = validate_coarse_operator(op, who))) return st;
  MUGIQ_REQUIRE(valid_op(opType), "%s: opType %d is none of M, Mdag, MdagM, MMdag, H", who, opType);
  if ((st = validate_coarse_vectors(src_h, nVec, op, who, "src"))) return st;
  if ((st = validate_coarse_vectors(dst_h, nVec, op, who, "dst"))) return st;
  for (int r = 0; r < nVec; r++) {
    uintptr_t a0, a1;
    coarse_span(dst_h[r], &a0, &a1);
    for (int q = 0; q < nVec; q++) {
      uintptr_t b0, b1;
      coarse_span(src_h[q], &b0, &b1);
      MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1), "%s: dst vector %d overlaps src vector %d", who, r, q);
    }
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  return coarse_apply(dst_h, src_h, nVec, op, opType, scale, s);
}

int mugiq_hip_coarse_apply_outputs(const MugiqHipCoarseOperator *op, int nVec) {
  const char *who = "coarseApplyOutputs";
  if (validate_coarse_operator(op, who)) return 0;
  if (nVec < 1) {
    set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: nVec = %d must be at least 1", who, nVec);
    return 0;
  }
  return apply_outputs_per_workgroup(op, nVec);
}

}  // extern "C"
