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
//
// A process grid (the ..._grid entry points): both kernels have a ghost path as a template flag -- a hop that leaves the
// rank reads the neighbour's rows (build) or vectors (apply) from a face the neighbour rank sent, and M^dag its matrix from the
// MugiqHipCoarseHalo -- behind pack kernels and one transfer group per launch.  Terms, products and their order do not change.
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

// The ghost path of a process grid, a template flag of both kernels: what a workgroup reads in place of the body when its hop leaves the
// rank -- a condition that is uniform over the workgroup, which owns one aggregate (build) or one coarse site (apply).  Without the flag
// the struct is empty and the kernel is the code it was.  Face indexing: MugiqHipCoarseHalo in include/mugiq_hip.h; [..][0] came from the
// backward neighbour (its high face), [..][1] from the forward one (its low face)
template <bool GHOST> struct BuildGhost {};
template <> struct BuildGhost<true> {
  const void *Vg[4][2];  // faces of V: [parity][(3s+c)*NV + j][faceCB]
  int part[4], faceCB[4];
};
template <bool GHOST> struct ApplyGhost {};
template <> struct ApplyGhost<true> {
  const void *vec[4][2];  // faces of the input vectors of the launch: [vector][parity][N][faceCB]
  const void *Y[4][2];    // MugiqHipCoarseHalo: Yback[mu] (Y+_mu of the backward neighbour's high face), Yfwd[mu] (Y-_mu of the forward one's low face)
  int part[4], faceCB[4];
};

template <typename FV, typename FG, bool GHOST>
__global__ __launch_bounds__(kCbThreads) void coarse_build_kernel(CoarseBuildArgs a, BuildGhost<GHOST> gh) {
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
        // GHOST: the hop leaves the rank -- the neighbour's rows wait in the face the neighbour rank sent (the link comes from the border)
        [[maybe_unused]] const void *Vn = a.V;
        [[maybe_unused]] int nstride = a.Vstride;
        [[maybe_unused]] int64_t nbase = npty * a.Vpo + nidx;
        if constexpr (GHOST) {
          if (gh.part[mu] && (fwd ? x[mu] + 1 == a.g.X[mu] : x[mu] == 0)) {
            Vn = gh.Vg[mu][fwd];
            nstride = gh.faceCB[mu];
            nbase = (int64_t)npty * 12 * NV * nstride + ghost_face_index_on_face(x, a.g.X, mu);
          }
        }
        for (int idx = t; idx < 8 * NV; idx += kCbThreads) {
          const int s = idx / N, rem = idx - s * N, Sp = rem / NV, jp = rem - Sp * NV;
          int ph, col;
          gamma_mu_row(mu, s, &ph, &col);
          const bool same = (s >> 1) == Sp;
          const int ss = same ? s : col;  // the spin of chirality Sp that (1 -+ g_mu) couples s to
          Cplx<double> T[3];
#pragma unroll
          for (int cp = 0; cp < 3; cp++) {
            Cplx<double> v;
            if constexpr (!GHOST) v = ld_wide<FV>(a.V, npty * a.Vpo + (int64_t)((3 * ss + cp) * NV + jp) * a.Vstride + nidx);
            else v = ld_wide<FV>(Vn, nbase + (int64_t)((3 * ss + cp) * NV + jp) * nstride);
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
                 hipStream_t stream, const BuildGhost<true> *gh = nullptr) {
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
  if (gh) hipLaunchKernelGGL((coarse_build_kernel<FV, FG, true>), grid, dim3(kCbThreads), lds, stream, a, *gh);
  else hipLaunchKernelGGL((coarse_build_kernel<FV, FG, false>), grid, dim3(kCbThreads), lds, stream, a, BuildGhost<false>{});
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
template <typename F, int DAG, int OUT, bool GHOST>
__global__ __launch_bounds__(kCaThreads) void coarse_apply_kernel(CoarseApplyArgs a, ApplyGhost<GHOST> gh) {
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
    int64_t mbase = ((int64_t)msite * 9 + mm) * N * N;
    const void *mptr = a.op;
    __syncthreads();  // the previous matrix is through
    bool staged = false;
    if constexpr (GHOST) {
      // the input site is on the neighbour rank: its vectors are in the face that rank sent, and the matrix M^dag wants in the halo
      if (m > 0 && gh.part[mu] && cc[mu] == (fwd ? a.Xc[mu] - 1 : 0)) {
        const int fcb = gh.faceCB[mu], fidx = ghost_face_index_on_face(cc, a.Xc, mu);
        const void *face = gh.vec[mu][fwd];
        for (int idx = t; idx < kCaRB * N; idx += kCaThreads) {
          const int v = idx / N, c = idx - v * N;
          in_s[idx] = ld_wide<F>(face, (((int64_t)min(n0 + v, a.nVec - 1) * 2 + npar) * N + c) * fcb + fidx);
        }
        if (DAG) {
          mptr = gh.Y[mu][fwd];
          mbase = ((int64_t)npar * fcb + fidx) * N * N;
        }
        staged = true;
      }
    }
    if (!staged)
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
            const Cplx<double> e = ld_wide<F>(mptr, mbase + (int64_t)r * N + c);
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
            const Cplx<double> e = ld_wide<F>(mptr, mbase + (int64_t)r * N + c);
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

template <typename F, int DAG, bool GHOST>
void launch_apply_form(int out, dim3 grid, size_t lds, hipStream_t stream, const CoarseApplyArgs &a, int N, const ApplyGhost<GHOST> &gh) {
  grid.z = (N + out - 1) / out;
  if (out == 16) hipLaunchKernelGGL((coarse_apply_kernel<F, DAG, 16, GHOST>), grid, dim3(kCaThreads), lds, stream, a, gh);
  else if (out == 32) hipLaunchKernelGGL((coarse_apply_kernel<F, DAG, 32, GHOST>), grid, dim3(kCaThreads), lds, stream, a, gh);
  else hipLaunchKernelGGL((coarse_apply_kernel<F, DAG, 64, GHOST>), grid, dim3(kCaThreads), lds, stream, a, gh);
}
template <bool GHOST>
void launch_apply_storage(int precision, int dagger, int out, dim3 grid, size_t lds, hipStream_t stream, const CoarseApplyArgs &a, int N,
                          const ApplyGhost<GHOST> &gh) {
  if (precision == 8 && !dagger) launch_apply_form<double, 0>(out, grid, lds, stream, a, N, gh);
  else if (precision == 8) launch_apply_form<double, 1>(out, grid, lds, stream, a, N, gh);
  else if (!dagger) launch_apply_form<float, 0>(out, grid, lds, stream, a, N, gh);
  else launch_apply_form<float, 1>(out, grid, lds, stream, a, N, gh);
}

// dst_i = scale [G5] M_c^(dag) src_i, i < n;  gh: the faces and halo matrices of a process grid (NULL: one domain)
int launch_apply(const MugiqHipCoarseField *dst, const MugiqHipCoarseField *src, int n, const MugiqHipCoarseOperator *op, int dagger, int gamma5,
                 double scale, hipStream_t stream, const ApplyGhost<true> *gh = nullptr) {
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
  if (gh) launch_apply_storage(op->precision, dagger, out, grid, lds, stream, a, N, *gh);
  else launch_apply_storage(op->precision, dagger, out, grid, lds, stream, a, N, ApplyGhost<false>{});
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

// ---- the faces of a process grid ----------------------------------------------------------------------------------------------------
// The face site (parity par, index f < faceCB) of axis mu, low (x[mu] = 0) or high (X[mu] - 1): its checkerboard index in the body.  The
// three other coordinates in lexicographic order, lowest axis fastest, halved (the lowest of them has an even extent, so the parity picks
// one of the pair 2 f, 2 f + 1): the inverse of ghost_face_index_on_face
__device__ inline int face_site_cb(const int X[4], int mu, int high, int par, int f) {
  int c[4], q = 2 * f, low = -1, sum = 0;
#pragma unroll
  for (int d = 0; d < 4; d++) {
    if (d == mu) {
      c[d] = high ? X[d] - 1 : 0;
    } else {
      c[d] = q % X[d];
      q /= X[d];
      if (low < 0) low = d;
    }
    sum += c[d];
  }
  c[low] += (par - sum) & 1;
  return lex_index(c, X) >> 1;
}

// Faces of fields stored as rows of sites (V: 12 n_vec rows; a coarse vector: N rows), for one body or a table of them:
// out[vector][parity][row][f] = body_vector[parity * po + row * stride + site(parity, f)].  One lane per (row, f), f fastest on both sides
struct FacePackArgs {
  const void *const *tab;  // device table of bodies (NULL: the one body `body`)
  const void *body;
  void *out;
  int rows, stride;
  int64_t po;
  int X[4], mu, high, faceCB;
};
template <typename F> __global__ __launch_bounds__(256) void face_pack_kernel(FacePackArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)a.rows * a.faceCB) return;
  const int row = (int)(idx / a.faceCB), f = (int)(idx - (int64_t)row * a.faceCB), par = blockIdx.y & 1;
  const void *src = a.tab ? as_constant(a.tab)[blockIdx.y >> 1] : a.body;
  const Cplx<double> v = ld_wide<F>(src, par * a.po + (int64_t)row * a.stride + face_site_cb(a.X, a.mu, a.high, par, f));
  st_round<F>(a.out, (int64_t)blockIdx.y * a.rows * a.faceCB + idx, v);
}

// Matrix m of every site of a face, matrix-contiguous: out[(parity * faceCB + f) * N^2 + e].  One workgroup per face site
struct MatrixPackArgs {
  const void *op;
  void *out;
  int NN, volumeCB, X[4], mu, high, faceCB, m;
};
template <typename F> __global__ __launch_bounds__(256) void matrix_face_pack_kernel(MatrixPackArgs a) {
  const int par = blockIdx.x / a.faceCB, f = blockIdx.x - par * a.faceCB;
  const int64_t sbase = (((int64_t)par * a.volumeCB + face_site_cb(a.X, a.mu, a.high, par, f)) * 9 + a.m) * a.NN, obase = (int64_t)blockIdx.x * a.NN;
  for (int e = threadIdx.x; e < a.NN; e += 256) st_round<F>(a.out, obase + e, ld_wide<F>(a.op, sbase + e));
}

// The send and receive buffers of one exchange: per partitioned axis the low face [0] and the high face [1] to send, and what arrives
// from the backward [0] and the forward [1] neighbour
struct FaceBuffers {
  unsigned char *send[4][2] = {}, *recv[4][2] = {};
  size_t bytes[4] = {0, 0, 0, 0};  // of one message
};
// ... carved from *cur, `cap[d]` bytes each (0: the axis is not partitioned); receive buffers only where recvToo
void carve_faces(FaceBuffers *b, unsigned char **cur, const size_t cap[4], bool recvToo) {
  for (int d = 0; d < 4; d++)
    for (int k = 0; k < (recvToo ? 4 : 2); k++) {
      if (cap[d] == 0) continue;
      (k < 2 ? b->send[d][k] : b->recv[d][k - 2]) = *cur;
      *cur += align256(cap[d]);
    }
}
// One transfer group: pack(d, high, send buffer) launches the pack kernel of a face; the high face goes forward and arrives, on the
// forward neighbour, from the backward one
template <typename Pack>
int exchange_faces(const MugiqHipComm *comm, const int part[4], const FaceBuffers &b, hipStream_t stream, const char *who, Pack &&pack) {
  int st;
  const bool grouped = comm->group_begin && comm->group_end;
  if (grouped && (st = comm->group_begin(comm->ctx))) return set_error(MUGIQ_HIP_ERROR_HIP, "%s: group_begin callback failed with status %d", who, st);
  for (int d = 0; d < 4; d++) {
    if (!part[d]) continue;
    for (int high = 0; high < 2; high++) {
      if ((st = pack(d, high, b.send[d][high]))) return st;
      if ((st = comm->sendrecv(comm->ctx, b.send[d][high], b.recv[d][1 - high], b.bytes[d], d, high ? +1 : -1, stream)))
        return set_error(MUGIQ_HIP_ERROR_HIP, "%s: halo sendrecv callback failed with status %d", who, st);
    }
  }
  if (grouped && (st = comm->group_end(comm->ctx, stream))) return set_error(MUGIQ_HIP_ERROR_HIP, "%s: group_end callback failed with status %d", who, st);
  return MUGIQ_HIP_SUCCESS;
}

template <typename F> int launch_face_pack(FacePackArgs a, int nBodies, hipStream_t stream) {
  const int64_t per = (int64_t)a.rows * a.faceCB;
  hipLaunchKernelGGL((face_pack_kernel<F>), dim3((unsigned)((per + 255) / 256), 2 * nBodies), dim3(256), 0, stream, a);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

bool any_partitioned(const int part[4]) { return part[0] || part[1] || part[2] || part[3]; }

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

int check_coarse_grid(const MugiqHipComm *comm, const MugiqHipCoarseOperator *op, const MugiqHipCoarseHalo *halo, int part[4], bool needSums,
                      const char *who) {
  int st;
  if ((st = check_comm(comm, part, needSums, who))) return st;
  if ((st = validate_coarse_operator(op, who))) return st;
  MUGIQ_REQUIRE(!any_partitioned(part) || halo != nullptr, "%s: the comm has a partitioned axis but the coarse halo is NULL", who);
  if (halo == nullptr) return MUGIQ_HIP_SUCCESS;
  MUGIQ_REQUIRE(halo->precision == op->precision && halo->nVec == op->nVec && halo->volumeCB == op->volumeCB,
                "%s: the coarse halo (precision %d, n_vec %d, volumeCB %d) does not belong to the coarse operator (precision %d, n_vec %d, volumeCB %d)", who,
                halo->precision, halo->nVec, halo->volumeCB, op->precision, op->nVec, op->volumeCB);
  for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(halo->X[d] == op->X[d], "%s: coarse halo X[%d] = %d, the coarse operator's is %d", who, d, halo->X[d], op->X[d]);
  for (int d = 0; d < 4; d++)
    MUGIQ_REQUIRE(!part[d] || (halo->dims[d] && halo->Yback[d] && halo->Yfwd[d]), "%s: dimension %d is partitioned but the coarse halo was not built for it",
                  who, d);
  return MUGIQ_HIP_SUCCESS;
}

// The work memory of coarse_apply_grid, from the start of the per-stream workspace: [the intermediate of a normal form, 8 vectors][per
// partitioned axis: two send and two receive faces of the most vectors one launch takes].  A function of the operator, the partitioned
// axes, the form and min(nVec, 8) alone
void coarse_grid_layout(CoarseGridLayout *L, const MugiqHipCoarseOperator *op, const int part[4], int opType, int nVec) {
  const int N = 2 * op->nVec, perLaunch = normal_op(opType) ? std::min(kCaRB, nVec) : nVec;
  const size_t cplx = 2 * (size_t)op->precision, one = normal_op(opType) ? align256((size_t)2 * N * op->volumeCB * cplx) : 0;
  *L = CoarseGridLayout{};
  L->intermediate = one;
  size_t at = kCaRB * one;
  for (int d = 0; d < 4; d++) {
    L->faceCB[d] = op->volumeCB / op->X[d];
    L->cap[d] = part[d] ? (size_t)perLaunch * 2 * N * L->faceCB[d] * cplx : 0;
    for (int k = 0; k < 4; k++) {  // send low, send high, receive backward, receive forward
      if (L->cap[d] == 0) continue;
      (k < 2 ? L->send[d][k] : L->recv[d][k - 2]) = at;
      at += align256(L->cap[d]);
    }
  }
  L->bytes = at;
}

// validated arguments.  Work memory (per-stream workspace): coarse_grid_layout.  Per launch: faces packed and exchanged (one group), then
// the kernel.  firstPacked: the send faces of the first launch are in place already (written by the caller into the buffers of
// coarse_grid_layout; nVec <= 8, one block): that launch exchanges without packing.  counts (may be NULL): exchanges and pack launches
// are added
int coarse_apply_grid(const MugiqHipCoarseField *dst, const MugiqHipCoarseField *src, int nVec, const MugiqHipCoarseOperator *op,
                      const MugiqHipCoarseHalo *halo, const int part[4], int opType, double scale, const MugiqHipComm *comm, hipStream_t stream,
                      bool firstPacked, CoarseGridCounts *counts) {
  if (!any_partitioned(part)) return coarse_apply(dst, src, nVec, op, opType, scale, stream);
  const char *who = "coarseApplyGrid";
  const int N = 2 * op->nVec;
  const size_t cplx = 2 * (size_t)op->precision;
  CoarseGridLayout L;
  coarse_grid_layout(&L, op, part, opType, nVec);
  const size_t one = L.intermediate;
  ApplyGhost<true> gh;
  for (int d = 0; d < 4; d++) {
    gh.part[d] = part[d];
    gh.faceCB[d] = L.faceCB[d];
    gh.Y[d][0] = part[d] ? halo->Yback[d] : nullptr;
    gh.Y[d][1] = part[d] ? halo->Yfwd[d] : nullptr;
  }
  void *ws = nullptr;
  if (int st = stream_workspace(&ws, L.bytes, stream)) return st;
  FaceBuffers fb;
  for (int d = 0; d < 4; d++)
    for (int k = 0; k < 2; k++) {
      if (L.cap[d] == 0) continue;
      fb.send[d][k] = static_cast<unsigned char *>(ws) + L.send[d][k];
      fb.recv[d][k] = static_cast<unsigned char *>(ws) + L.recv[d][k];
    }
  for (int d = 0; d < 4; d++) gh.vec[d][0] = fb.recv[d][0], gh.vec[d][1] = fb.recv[d][1];

  int launches = 0;
  auto simple = [&](const MugiqHipCoarseField *d_, const MugiqHipCoarseField *s_, int n, int dagger, int gamma5, double f) -> int {
    std::vector<const void *> host(2 * (size_t)n);  // (the size of launch_apply's table, so the buffer stays where it is)
    for (int i = 0; i < n; i++) host[i] = host[n + i] = s_[i].data;
    void *dev = nullptr;
    if (int st = upload_table(&dev, host.data(), host.size() * sizeof(void *), stream)) return st;
    for (int d = 0; d < 4; d++) fb.bytes[d] = part[d] ? (size_t)n * 2 * N * gh.faceCB[d] * cplx : 0;
    const bool packed = firstPacked && launches == 0;
    launches++;
    int st = exchange_faces(comm, part, fb, stream, who, [&](int d, int high, unsigned char *send) -> int {
      if (packed) return MUGIQ_HIP_SUCCESS;
      if (counts) counts->packLaunches++;
      FacePackArgs p{static_cast<const void *const *>(dev), nullptr, send, N, s_[0].stride, s_[0].parity_offset, {op->X[0], op->X[1], op->X[2], op->X[3]}, d, high, gh.faceCB[d]};
      return with_storage(op->precision, [&](auto fs) { return launch_face_pack<decltype(fs)>(p, n, stream); });
    });
    if (st) return st;
    if (counts) counts->exchanges++;
    return launch_apply(d_, s_, n, op, dagger, gamma5, f, stream, &gh);
  };
  MugiqHipCoarseField tmp[kCaRB];
  if (!normal_op(opType)) return apply_form(opType, simple, dst, src, tmp, nVec, scale);
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

}  // extern "C"

namespace {

// The faces of V to the neighbours (one group), into ws: the ghost arguments of the build
int exchange_transfer_faces(BuildGhost<true> *gh, FaceBuffers *fb, const MugiqHipTransfer *T, const int part[4], const MugiqHipComm *comm,
                            hipStream_t stream, const char *who) {
  const int rows = 12 * T->nVec;
  for (int d = 0; d < 4; d++) {
    gh->part[d] = part[d];
    gh->Vg[d][0] = fb->recv[d][0], gh->Vg[d][1] = fb->recv[d][1];
  }
  return exchange_faces(comm, part, *fb, stream, who, [&](int d, int high, unsigned char *send) {
    FacePackArgs p{nullptr, T->V, send, rows, T->stride, T->parity_offset, {T->X[0], T->X[1], T->X[2], T->X[3]}, d, high, gh->faceCB[d]};
    return with_storage(T->precision, [&](auto fv) { return launch_face_pack<decltype(fv)>(p, 1, stream); });
  });
}

// mugiq_hip_compute_coarse_operator (grid false: one domain, or MUGIQ_HIP_ERROR_UNSUPPORTED) and ..._grid
int compute_coarse_operator(MugiqHipCoarseOperator *op, const MugiqHipCoarseHalo *halo, const MugiqHipTransfer *transfer, const MugiqHipGaugeField *gauge,
                            const MugiqHipCloverField *clover, double kappa, const MugiqHipComm *comm, void *stream, const char *who, bool grid) {
  // ---- validation, before any device work
  MUGIQ_REQUIRE(op != nullptr && transfer != nullptr, "%s: NULL argument", who);
  int st, part[4] = {0, 0, 0, 0};
  if (grid) {
    if ((st = check_coarse_grid(comm, op, halo, part, false, who))) return st;
  } else {
    if ((st = check_single_domain(comm, who))) return st;
    if ((st = validate_coarse_operator(op, who))) return st;
  }
  MUGIQ_REQUIRE(transfer->V != nullptr, "%s: transfer / null vectors are NULL", who);
  if ((st = validate_transfer_operator(transfer, op, who))) return st;
  if ((st = check_gauge(gauge, transfer->X, part, who))) return st;
  const TransferGeom g = transfer_geom(*transfer);
  if (clover) {
    if ((st = validate_clover(clover, transfer->X, g.volumeCB, who))) return st;
    MUGIQ_REQUIRE(clover->precision == gauge->precision, "%s: clover precision %d differs from the gauge precision %d", who, clover->precision, gauge->precision);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  if (!any_partitioned(part)) {
    st = with_storage(transfer->precision, gauge->precision, [&](auto fv, auto fg) {
      return launch_build<decltype(fv), decltype(fg)>(op, transfer, gauge, clover, kappa, s);
    });
    if (st) return st;
    op->kappa = kappa;
    op->hasClover = clover ? 1 : 0;
    return MUGIQ_HIP_SUCCESS;
  }
  // ---- a process grid.  Work memory (per-stream workspace): per partitioned axis two send and two receive faces of V, two send faces of Y
  const size_t cplx = 2 * (size_t)op->precision, NN = (size_t)4 * op->nVec * op->nVec;
  BuildGhost<true> gh;
  size_t capV[4], capY[4], total = 0;
  int faceCBc[4];
  for (int d = 0; d < 4; d++) {
    gh.faceCB[d] = g.volumeCB / transfer->X[d];
    faceCBc[d] = op->volumeCB / op->X[d];
    capV[d] = part[d] ? (size_t)2 * 12 * transfer->nVec * gh.faceCB[d] * cplx : 0;
    capY[d] = part[d] ? (size_t)2 * faceCBc[d] * NN * cplx : 0;
    total += 4 * align256(capV[d]) + 2 * align256(capY[d]);
  }
  void *ws = nullptr;
  if ((st = stream_workspace(&ws, total, s))) return st;
  unsigned char *cur = static_cast<unsigned char *>(ws);
  FaceBuffers fv, fy;
  carve_faces(&fv, &cur, capV, true);
  carve_faces(&fy, &cur, capY, false);
  for (int d = 0; d < 4; d++) {
    fv.bytes[d] = capV[d], fy.bytes[d] = capY[d];
    fy.recv[d][0] = static_cast<unsigned char *>(halo->Yback[d]), fy.recv[d][1] = static_cast<unsigned char *>(halo->Yfwd[d]);
  }
  if ((st = exchange_transfer_faces(&gh, &fv, transfer, part, comm, s, who))) return st;
  st = with_storage(transfer->precision, gauge->precision, [&](auto fv_, auto fg) {
    return launch_build<decltype(fv_), decltype(fg)>(op, transfer, gauge, clover, kappa, s, &gh);
  });
  if (st) return st;
  // Y+_mu of the high face goes forward (the neighbour's Yback), Y-_mu of the low face backward (its Yfwd)
  st = exchange_faces(comm, part, fy, s, who, [&](int d, int high, unsigned char *send) -> int {
    MatrixPackArgs p{op->data, send, (int)NN, op->volumeCB, {op->X[0], op->X[1], op->X[2], op->X[3]}, d, high, faceCBc[d], high ? 1 + 2 * d : 2 + 2 * d};
    with_storage(op->precision, [&](auto f) {
      hipLaunchKernelGGL((matrix_face_pack_kernel<decltype(f)>), dim3(2 * faceCBc[d]), dim3(256), 0, s, p);
    });
    MUGIQ_CHECK_HIP(hipGetLastError());
    return MUGIQ_HIP_SUCCESS;
  });
  if (st) return st;
  op->kappa = kappa;
  op->hasClover = clover ? 1 : 0;
  return MUGIQ_HIP_SUCCESS;
}

size_t halo_face_elems(const int X[4], int nVec, int d) {
  size_t vol = 1;
  for (int k = 0; k < 4; k++) vol *= (size_t)X[k];
  return vol / (size_t)X[d] * 4 * (size_t)nVec * (size_t)nVec;  // both parities of the face x N^2
}

}  // namespace

extern "C" {

int mugiq_hip_compute_coarse_operator(MugiqHipCoarseOperator *op, const MugiqHipTransfer *transfer, const MugiqHipGaugeField *gauge,
                                      const MugiqHipCloverField *clover, double kappa, const MugiqHipComm *comm, void *stream) {
  return compute_coarse_operator(op, nullptr, transfer, gauge, clover, kappa, comm, stream, "computeCoarseOperator", false);
}

int mugiq_hip_compute_coarse_operator_grid(MugiqHipCoarseOperator *op, const MugiqHipCoarseHalo *halo, const MugiqHipTransfer *transfer,
                                           const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover, double kappa,
                                           const MugiqHipComm *comm, void *stream) {
  return compute_coarse_operator(op, halo, transfer, gauge, clover, kappa, comm, stream, "computeCoarseOperatorGrid", true);
}

size_t mugiq_hip_coarse_halo_bytes(const int X[4], int nVec, int precision, const int dims[4]) {
  if (!X || !dims || nVec < 1 || nVec > kTransferMaxNV || (precision != 4 && precision != 8)) return 0;
  size_t bytes = 0;
  for (int d = 0; d < 4; d++) {
    if (X[d] <= 0 || (X[d] & 1)) return 0;
    if (dims[d]) bytes += 2 * halo_face_elems(X, nVec, d) * 2 * (size_t)precision;  // Yback and Yfwd
  }
  return bytes;
}

int mugiq_hip_alloc_coarse_halo(MugiqHipCoarseHalo *halo, const MugiqHipCoarseOperator *op, const int dims[4]) {
  const char *who = "allocCoarseHalo";
  MUGIQ_REQUIRE(halo && op && dims, "%s: NULL argument", who);
  MugiqHipCoarseOperator geom = *op;
  geom.data = reinterpret_cast<void *>(uintptr_t(16));  // geometry only: never read
  if (int st = validate_coarse_operator(&geom, who)) return st;
  halo->precision = op->precision, halo->nVec = op->nVec, halo->volumeCB = op->volumeCB;
  for (int d = 0; d < 4; d++) {
    halo->X[d] = op->X[d];
    halo->dims[d] = dims[d] ? 1 : 0;
    halo->Yback[d] = halo->Yfwd[d] = nullptr;
  }
  for (int d = 0; d < 4; d++) {
    if (!halo->dims[d]) continue;
    const size_t bytes = halo_face_elems(op->X, op->nVec, d) * 2 * (size_t)op->precision;
    for (void **p : {&halo->Yback[d], &halo->Yfwd[d]}) {
      hipError_t e = hipMalloc(p, bytes);
      if (e == hipSuccess) e = hipMemset(*p, 0, bytes);
      else *p = nullptr;
      if (e != hipSuccess) {  // the caller gets a complete halo or nothing
        (void)mugiq_hip_free_coarse_halo(halo);
        return set_error(MUGIQ_HIP_ERROR_HIP, "%s: allocating %zu bytes failed: %s", who, bytes, hipGetErrorString(e));
      }
    }
  }
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_free_coarse_halo(MugiqHipCoarseHalo *halo) {
  if (!halo) return MUGIQ_HIP_SUCCESS;
  for (int d = 0; d < 4; d++)
    for (void **p : {&halo->Yback[d], &halo->Yfwd[d]}) {
      if (*p) MUGIQ_CHECK_HIP(hipFree(*p));
      *p = nullptr;
    }
  return MUGIQ_HIP_SUCCESS;
}

}  // extern "C"

namespace {

// mugiq_hip_coarse_apply (grid false: one domain, or MUGIQ_HIP_ERROR_UNSUPPORTED) and ..._grid
int coarse_apply_entry(const MugiqHipCoarseField *dst_h, const MugiqHipCoarseField *src_h, int nVec, const MugiqHipCoarseOperator *op,
                       const MugiqHipCoarseHalo *halo, int opType, double scale, const MugiqHipComm *comm, void *stream, const char *who, bool grid) {
  MUGIQ_REQUIRE(dst_h != nullptr && src_h != nullptr && nVec >= 1, "%s: NULL / empty argument", who);
  int st, part[4] = {0, 0, 0, 0};
  if (grid) {
    if ((st = check_coarse_grid(comm, op, halo, part, false, who))) return st;
  } else {
    if ((st = check_single_domain(comm, who))) return st;
    if ((st = validate_coarse_operator(op, who))) return st;
  }
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
  return coarse_apply_grid(dst_h, src_h, nVec, op, halo, part, opType, scale, comm, s);  // (nothing partitioned: coarse_apply)
}

}  // namespace

extern "C" {

int mugiq_hip_coarse_apply(const MugiqHipCoarseField *dst_h, const MugiqHipCoarseField *src_h, int nVec, const MugiqHipCoarseOperator *op, int opType,
                           double scale, const MugiqHipComm *comm, void *stream) {
  return coarse_apply_entry(dst_h, src_h, nVec, op, nullptr, opType, scale, comm, stream, "coarseApply", false);
}

int mugiq_hip_coarse_apply_grid(const MugiqHipCoarseField *dst_h, const MugiqHipCoarseField *src_h, int nVec, const MugiqHipCoarseOperator *op,
                                const MugiqHipCoarseHalo *halo, int opType, double scale, const MugiqHipComm *comm, void *stream) {
  return coarse_apply_entry(dst_h, src_h, nVec, op, halo, opType, scale, comm, stream, "coarseApplyGrid", true);
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
