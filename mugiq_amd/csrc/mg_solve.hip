// A flexible GCR on the fine Wilson(-clover) operator, preconditioned by one two-grid cycle K: MR smoothing and a coarse-grid correction
// through R, a fixed number of GCR steps on the explicit coarse operator, and P.  Definitions (MR step, GCRfix, K, the outer solve), limits
// and work memory: mugiq_hip_mg_solve in include/mugiq_hip.h.  The stencil, R, P and the coarse application are the library's own, called
// below their C entries (csrc/internal.h) on arguments checked once, up front; what is new here are the Krylov kernels between them, on every level.  With a second coarse level the
// level-1 solve becomes a flexible GCR preconditioned by a cycle of its own through the coarsest operator (K^(3), the *_levels entry
// points).  The coarse levels are a chain (MgCoarse, MgSolver::coarse): MgSolver::cycle is K with the level abstracted, its correction
// restricts to the next level, solves there (MgSolver::solve: GCRfix on the last level, the flexible GCR above it) and prolongs back.
// With a deflation space for the last level (the *_levels_deflated entry points) its GCRfix starts from the projection on the space
// (csrc/mg_deflate.hip, called through csrc/mg_common.h); without one nothing here takes another path.
// On a process grid (the *_grid entry points: two-grid, fp64) M and M_c exchange halos and every final sum is completed over the ranks on
// the device: the rank table, its ring gather and mg_rank_sum_kernel (MgRankSum).  One rank makes no such sum.
//
// One set of kernels serves both levels and both storages: a field is a list of rows of complex numbers (MgLayout; fine FLOAT2: 12 rows of
// volumeCB per parity, fine FLOAT4: 6 rows of 2 volumeCB, coarse: 2 n_vec rows of volumeCB_c) stored as Cplx<F>, F = double or float.  Every
// lane takes one whole complex number per access (16 bytes in fp64, 8 bytes in fp32, consecutive along a row: a wave's access is one
// contiguous run of 1 KiB or 512 B), widens it to fp64 on the load (ld_wide, csrc/mg_common.h), forms every product and every sum in fp64 and
// rounds once on the store (st_round); the scalars -- partial sums, Gram-Schmidt coefficients, nu, alpha -- are fp64 in device memory for either storage.  The
// element a lane takes does not depend on F, so the order of every sum is the same in both storages, and no alignment beyond that of one
// complex number is asked of a row (an odd stride or a row that cuts a wave needs no peeling).  Pads are never touched.  blockIdx.y is
// the right-hand side; a right-hand side whose `active` bit is clear is not touched.  Every sum is taken per lane over its elements in
// ascending order, over the wave by shuffles, over the workgroup's four waves and then over the workgroups by mg_final_sum_kernel, each in a fixed order that depends on the shape of the field alone: no atomics, two
// runs give the same bits, and a right-hand side has the same sums wherever it stands in a block.
//
// The Krylov directions of a level lie behind one base pointer, direction j of right-hand side v at (j nb + v) vecElems, so that a kernel
// reaches all of them without a pointer table.  Scalars never leave the device inside K: mg_final_sum_kernel turns the partial sums into
// the Gram-Schmidt coefficients, into (nu, alpha) of a GCR step or into alpha of an MR step, and the next kernel reads them from memory.
// The host reads only the squared residual norms of the outer iteration (and ||b||^2 and the true residual, once per block each).
#include "mg_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace mugiq {
namespace {

constexpr int kMgMaxDir = 16;     // stored directions of a level
constexpr int kMgThreads = 256;
constexpr int kMgMaxGroups = 256; // workgroups of a pass per right-hand side: the partial sums mg_final_sum_kernel adds up
constexpr int kMgSlots = 32;      // doubles per right-hand side and workgroup: up to 15 complex coefficients, or 3 sums
static_assert(2 * (kMgMaxDir - 1) <= kMgSlots && kMgBlock * kMgSlots == kMgThreads, "mg_final_sum_kernel: one lane per (right-hand side, slot)");

typedef Cplx<double> Z;

// v[0 .. nUsed) summed over the workgroup -> out[0 .. nUsed): down the wave by shuffles, then the four waves in ascending order
template <int NS> __device__ inline void mg_group_sum(double (&v)[NS], int nUsed, double *out) {
  __shared__ double sh[kMgThreads / 64][NS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int s = 0; s < NS; s++) {
    if (s < nUsed) {
      double x = v[s];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
      if (lane == 0) sh[w][s] = x;
    }
  }
  __syncthreads();
  if (t < nUsed) out[t] = ((sh[0][t] + sh[1][t]) + sh[2][t]) + sh[3][t];
}

// multi-dot: c_j = <q_j, q_k> for all j < k, from the q_k the operator left (classical Gram-Schmidt): slots (2j, 2j + 1)
template <typename F, typename I>
__global__ __launch_bounds__(kMgThreads) void mg_multidot_kernel(const Cplx<F> *Q, int64_t vecElems, int nb, int k, MgLayout L, unsigned active, double *partial) {
  const int v = blockIdx.y;
  if (!((active >> v) & 1u)) return;
  double acc[kMgSlots];
#pragma unroll
  for (int s = 0; s < kMgSlots; s++) acc[s] = 0.0;
  const Cplx<F> *qk = Q + ((int64_t)k * nb + v) * vecElems;
  for (I e = (I)blockIdx.x * kMgThreads + threadIdx.x; e < (I)L.total; e += (I)gridDim.x * kMgThreads) {
    const int64_t off = mg_offset<I>(L, e);
    const Z q = ld_wide(qk, off);
#pragma unroll
    for (int j = 0; j < kMgMaxDir - 1; j++) {
      if (j < k) {
        const Z a = ld_wide(Q + ((int64_t)j * nb + v) * vecElems, off);
        acc[2 * j] = fma(a.re, q.re, acc[2 * j]);
        acc[2 * j] = fma(a.im, q.im, acc[2 * j]);
        acc[2 * j + 1] = fma(a.re, q.im, acc[2 * j + 1]);
        acc[2 * j + 1] = fma(-a.im, q.re, acc[2 * j + 1]);
      }
    }
  }
  mg_group_sum<kMgSlots>(acc, 2 * k, partial + ((size_t)v * gridDim.x + blockIdx.x) * kMgSlots);
}

// multi-axpy: p_k -= sum_j c_j p_j, q_k -= sum_j c_j q_j with c from device memory; in the same pass ||q_k||^2 (slot 0) and <q_k, r>
// (slots 1, 2) of the orthogonalised q_k
template <typename F, typename I>
__global__ __launch_bounds__(kMgThreads) void mg_multiaxpy_kernel(Cplx<F> *P, Cplx<F> *Q, int64_t vecElems, int nb, int k, MgVecs<F> R, const double *coef, MgLayout L,
                                                                 unsigned active, double *partial) {
  const int v = blockIdx.y;
  if (!((active >> v) & 1u)) return;
  double c[2 * (kMgMaxDir - 1)];
#pragma unroll
  for (int s = 0; s < 2 * (kMgMaxDir - 1); s++) c[s] = s < 2 * k ? coef[v * kMgSlots + s] : 0.0;
  double acc[3] = {0.0, 0.0, 0.0};
  Cplx<F> *pk = P + ((int64_t)k * nb + v) * vecElems, *qk = Q + ((int64_t)k * nb + v) * vecElems;
  for (I e = (I)blockIdx.x * kMgThreads + threadIdx.x; e < (I)L.total; e += (I)gridDim.x * kMgThreads) {
    const int64_t off = mg_offset<I>(L, e);
    Z q = ld_wide(qk, off);
    if (k > 0) {
      Z p = ld_wide(pk, off);
#pragma unroll
      for (int j = 0; j < kMgMaxDir - 1; j++) {
        if (j < k) {
          const Z cj{-c[2 * j], -c[2 * j + 1]};
          cmadd(p, cj, ld_wide(P + ((int64_t)j * nb + v) * vecElems, off));
          cmadd(q, cj, ld_wide(Q + ((int64_t)j * nb + v) * vecElems, off));
        }
      }
      st_round(pk, off, p);
      st_round(qk, off, q);
    }
    const Z r = ld_wide(R.p[v], off);
    acc[0] = fma(q.re, q.re, acc[0]);
    acc[0] = fma(q.im, q.im, acc[0]);
    acc[1] = fma(q.re, r.re, acc[1]);
    acc[1] = fma(q.im, r.im, acc[1]);
    acc[2] = fma(q.re, r.im, acc[2]);
    acc[2] = fma(-q.im, r.re, acc[2]);
  }
  mg_group_sum<3>(acc, 3, partial + ((size_t)v * gridDim.x + blockIdx.x) * kMgSlots);
}

// update: p_k /= nu, q_k /= nu (nu = 0: a zero direction), x += alpha p_k (xZero: x = alpha p_k), r -= alpha q_k, ||r||^2 into slot 0;
// sc[4 v] = (nu, Re alpha, Im alpha) from mg_final_sum_kernel.  Pnext != NULL: the new r is also the next direction p_{k+1} (GCRfix)
template <typename F, typename I>
__global__ __launch_bounds__(kMgThreads) void mg_update_kernel(Cplx<F> *P, Cplx<F> *Q, int64_t vecElems, int nb, int k, MgVecs<F> X, MgVecs<F> R, const double *sc, int xZero,
                                                              Cplx<F> *Pnext, MgLayout L, unsigned active, double *partial) {
  const int v = blockIdx.y;
  if (!((active >> v) & 1u)) return;
  const double nu = sc[4 * v];
  const Z alpha{sc[4 * v + 1], sc[4 * v + 2]}, malpha{-alpha.re, -alpha.im};
  double acc[1] = {0.0};
  Cplx<F> *pk = P + ((int64_t)k * nb + v) * vecElems, *qk = Q + ((int64_t)k * nb + v) * vecElems;
  Cplx<F> *pn = Pnext ? Pnext + ((int64_t)(k + 1) * nb + v) * vecElems : nullptr;
  for (I e = (I)blockIdx.x * kMgThreads + threadIdx.x; e < (I)L.total; e += (I)gridDim.x * kMgThreads) {
    const int64_t off = mg_offset<I>(L, e);
    Z p = ld_wide(pk, off), q = ld_wide(qk, off);
    if (nu > 0.0) {
      p = Z{p.re / nu, p.im / nu};
      q = Z{q.re / nu, q.im / nu};
    } else {
      p = q = Z{0.0, 0.0};
    }
    st_round(pk, off, p);
    st_round(qk, off, q);
    Z x = xZero ? Z{0.0, 0.0} : ld_wide(X.p[v], off);
    cmadd(x, alpha, p);
    st_round(X.p[v], off, x);
    Z r = ld_wide(R.p[v], off);
    cmadd(r, malpha, q);
    st_round(R.p[v], off, r);
    if (pn) st_round(pn, off, r);
    acc[0] = fma(r.re, r.re, acc[0]);
    acc[0] = fma(r.im, r.im, acc[0]);
  }
  mg_group_sum<1>(acc, 1, partial + ((size_t)v * gridDim.x + blockIdx.x) * kMgSlots);
}

// <t, s> into slots 0, 1 and <t, t> into slot 2 (an MR step; with t = s: a norm)
template <typename F, typename I> __global__ __launch_bounds__(kMgThreads) void mg_dot2_kernel(MgVecs<F> T, MgVecs<F> S, MgLayout L, unsigned active, double *partial) {
  const int v = blockIdx.y;
  if (!((active >> v) & 1u)) return;
  double acc[3] = {0.0, 0.0, 0.0};
  for (I e = (I)blockIdx.x * kMgThreads + threadIdx.x; e < (I)L.total; e += (I)gridDim.x * kMgThreads) {
    const int64_t off = mg_offset<I>(L, e);
    const Z t = ld_wide(T.p[v], off), s = ld_wide(S.p[v], off);
    acc[0] = fma(t.re, s.re, acc[0]);
    acc[0] = fma(t.im, s.im, acc[0]);
    acc[1] = fma(t.re, s.im, acc[1]);
    acc[1] = fma(-t.im, s.re, acc[1]);
    acc[2] = fma(t.re, t.re, acc[2]);
    acc[2] = fma(t.im, t.im, acc[2]);
  }
  mg_group_sum<3>(acc, 3, partial + ((size_t)v * gridDim.x + blockIdx.x) * kMgSlots);
}

// the update of an MR step: z += alpha s (zZero: z = alpha s), sOut = s - alpha t (sOut NULL: the last step of K, s is not needed again);
// sc[4 v] = (Re alpha, Im alpha) from mg_final_sum_kernel.  sOut may be s
template <typename F, typename I>
__global__ __launch_bounds__(kMgThreads) void mg_mr_update_kernel(MgVecs<F> Zv, MgVecs<F> S, MgVecs<F> T, MgVecs<F> SOut, const double *sc, int zZero, int writeS,
                                                                 MgLayout L, unsigned active) {
  const int v = blockIdx.y;
  if (!((active >> v) & 1u)) return;
  const Z alpha{sc[4 * v], sc[4 * v + 1]}, malpha{-alpha.re, -alpha.im};
  for (I e = (I)blockIdx.x * kMgThreads + threadIdx.x; e < (I)L.total; e += (I)gridDim.x * kMgThreads) {
    const int64_t off = mg_offset<I>(L, e);
    Z s = ld_wide(S.p[v], off);
    Z z = zZero ? Z{0.0, 0.0} : ld_wide(Zv.p[v], off);
    cmadd(z, alpha, s);
    st_round(Zv.p[v], off, z);
    if (writeS) {
      cmadd(s, malpha, ld_wide(T.p[v], off));
      st_round(SOut.p[v], off, s);
    }
  }
}

// c = sa a + sb b on the elements (a or b NULL: that term is zero; c may be a or b)
template <typename F, typename I>
__global__ __launch_bounds__(kMgThreads) void mg_axpby_kernel(MgVecs<F> C, MgVecs<F> A, double sa, MgVecs<F> B, double sb, MgLayout L, unsigned active) {
  const int v = blockIdx.y;
  if (!((active >> v) & 1u)) return;
  for (I e = (I)blockIdx.x * kMgThreads + threadIdx.x; e < (I)L.total; e += (I)gridDim.x * kMgThreads) {
    const int64_t off = mg_offset<I>(L, e);
    Z o{0.0, 0.0};
    if (A.p[v]) {
      const Z a = ld_wide(A.p[v], off);
      o = Z{sa * a.re, sa * a.im};
    }
    if (B.p[v]) {
      const Z b = ld_wide(B.p[v], off);
      o.re = fma(sb, b.re, o.re);
      o.im = fma(sb, b.im, o.im);
    }
    st_round(C.p[v], off, o);
  }
}

// d = s on the elements, between two storages and two layouts of the same rows (Ld.nRows == Ls.nRows, Ld.rowLen == Ls.rowLen): the
// precision hand-over of the mixed solve, and the copy of V between two transfers.  fp64 -> fp32 rounds to nearest even, once (what
// numpy's astype(complex64) does); fp32 -> fp64 is exact.  Pads of neither side are touched
template <typename FD, typename FS, typename I>
__global__ __launch_bounds__(kMgThreads) void mg_convert_kernel(MgVecs<FD> D, MgVecs<FS> S, MgLayout Ld, MgLayout Ls, unsigned active) {
  const int v = blockIdx.y;
  if (!((active >> v) & 1u)) return;
  for (I e = (I)blockIdx.x * kMgThreads + threadIdx.x; e < (I)Ls.total; e += (I)gridDim.x * kMgThreads)
    st_round(D.p[v], mg_offset<I>(Ld, e), ld_wide(S.p[v], mg_offset<I>(Ls, e)));
}

// The sums of the last pass over its workgroups, in ascending order, one lane per (right-hand side, slot), and what the next kernel needs
// of them.  kMgFinRaw: res[4 v + s] = sum s, s < 4 (what the host reads);  kMgFinCoef: coef[32 v + s] = sum s;
// kMgFinNorm (after mg_multiaxpy_kernel): sc[4 v] = (nu = sqrt ||q||^2, <q, r> / nu), zero for nu = 0;
// kMgFinMr (after mg_dot2_kernel): sc[4 v] = omega <t, s> / <t, t>, zero for <t, t> = 0.
// kMgFinTable (a rank of a process grid): the raw sums go into this rank's entry `mine` of the rank table [rank][kMgBlock][kMgSlots] and
// nothing else is written; the entries of all ranks are then gathered and mg_rank_sum_kernel applies the mode to their sum
enum { kMgFinRaw = 0, kMgFinCoef = 1, kMgFinNorm = 2, kMgFinMr = 3, kMgFinTable = 4 };
// what a mode makes of the sums: lane t = (v, s) holds sum s of right-hand side v in `a`, all of them are in `sum` (after a barrier).
// The guards nu > 0 and <t, t> > 0 act on the sums they are handed: on a process grid those over all ranks
__device__ inline void mg_sum_epilogue(int mode, double a, const double (*sum)[kMgSlots], int t, int v, int s, double omega, double *coef, double *sc,
                                       double *res) {
  if (mode == kMgFinCoef) {
    coef[t] = a;
  } else if (mode == kMgFinRaw) {
    if (s < 4) res[4 * v + s] = a;
  } else if (s == 0) {
    if (mode == kMgFinNorm) {
      const double nu = sqrt(sum[v][0]);
      sc[4 * v] = nu;
      sc[4 * v + 1] = nu > 0.0 ? sum[v][1] / nu : 0.0;
      sc[4 * v + 2] = nu > 0.0 ? sum[v][2] / nu : 0.0;
    } else {
      const double d = sum[v][2];
      sc[4 * v] = d > 0.0 ? omega * sum[v][0] / d : 0.0;
      sc[4 * v + 1] = d > 0.0 ? omega * sum[v][1] / d : 0.0;
    }
  }
}
__global__ __launch_bounds__(kMgThreads) void mg_final_sum_kernel(const double *partial, int nGroups, int nUsed, unsigned active, int mode, double omega,
                                                                 double *coef, double *sc, double *res, double *mine) {
  __shared__ double sum[kMgBlock][kMgSlots];
  const int t = threadIdx.x, v = t / kMgSlots, s = t - v * kMgSlots;
  double a = 0.0;
  if (((active >> v) & 1u) && s < nUsed)
    for (int g = 0; g < nGroups; g++) a += partial[((size_t)v * nGroups + g) * kMgSlots + s];
  if (mode == kMgFinTable) {  // (uniform over the workgroup)
    mine[t] = a;
    return;
  }
  sum[v][s] = a;
  __syncthreads();
  mg_sum_epilogue(mode, a, sum, t, v, s, omega, coef, sc, res);
}
// The sum over the ranks: one workgroup, lane t = (right-hand side, slot) adds entry t of table[0 .. size) in ascending rank order -- the
// same additions on every rank, so every rank holds the same bits -- and applies `mode` to the sums.  A slot or a right-hand side the
// local pass did not use is zero in every entry
__global__ __launch_bounds__(kMgThreads) void mg_rank_sum_kernel(const double *table, int size, int mode, double omega, double *coef, double *sc, double *res) {
  __shared__ double sum[kMgBlock][kMgSlots];
  const int t = threadIdx.x, v = t / kMgSlots, s = t - v * kMgSlots;
  double a = 0.0;
  for (int r = 0; r < size; r++) a += table[(size_t)r * kMgThreads + t];
  sum[v][s] = a;
  __syncthreads();
  mg_sum_epilogue(mode, a, sum, t, v, s, omega, coef, sc, res);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
MgLayout fine_layout(const MugiqHipSpinorField &f) {
  MgLayout L;
  const bool f2 = f.field_order == 2;
  L.nRows = f2 ? 12 : 6;
  L.rowLen = f2 ? f.volumeCB : (int64_t)2 * f.volumeCB;
  L.rowStride = f2 ? f.stride : (int64_t)2 * f.stride;
  L.po = f.parity_offset;
  L.total = 2 * L.nRows * L.rowLen;
  return L;
}
// rows of V: a finest-level transfer has 12 n_vec of them per parity, a coarse -> coarse one parity_offset / stride (2 nc n_vec, no gap)
MgLayout transfer_layout(const MugiqHipTransfer &T) {
  MgLayout L;
  L.nRows = T.spinBlockSize == 2 ? 12 * T.nVec : (int)(T.parity_offset / T.stride);
  L.rowLen = ((int64_t)T.X[0] * T.X[1] * T.X[2] * T.X[3]) / 2;
  L.rowStride = T.stride;
  L.po = T.parity_offset;
  L.total = 2 * L.nRows * L.rowLen;
  return L;
}
template <typename F> size_t fine_bytes(const MugiqHipSpinorField &f) { return align256((size_t)2 * (size_t)f.parity_offset * sizeof(Cplx<F>)); }
template <typename F> size_t coarse_bytes(const MugiqHipCoarseField &f) { return align256((size_t)2 * (size_t)f.parity_offset * sizeof(Cplx<F>)); }
size_t scalar_bytes() { return align256(sizeof(double) * ((size_t)kMgBlock * kMgMaxGroups * kMgSlots + kMgBlock * kMgSlots + 2 * 4 * kMgBlock)); }

// The messages of the ring gather that completes a rank table (mugiq_hip_mg_rank_sum_plan): over every axis of extent n > 1, t first,
// n - 1 calls of sendrecv(.., d, +1, ..); call k sends the run of coordinate (c - k + 1) mod n and receives that of (c - k) mod n.  A run
// are the entries of the ranks that share the coordinates of the axes still to come: with x slowest and t fastest one contiguous piece
int rank_sum_plan(const int grid[4], const int coord[4], int maxOps, int *dim, int *sendEntry, int *recvEntry, int *entries) {
  int nMsg = 0, run = 1;
  for (int d = 3; d >= 0; d--) {
    const int n = grid[d], c = coord[d];
    int base = 0;
    for (int e = 0; e < 4; e++) base = base * grid[e] + (e < d ? coord[e] : 0);
    for (int k = 1; k < n; k++, nMsg++) {
      if (nMsg >= maxOps) continue;
      if (dim) dim[nMsg] = d;
      if (sendEntry) sendEntry[nMsg] = base + ((c - k + 1 + n) % n) * run;
      if (recvEntry) recvEntry[nMsg] = base + ((c - k + n) % n) * run;
      if (entries) entries[nMsg] = run;
    }
    run *= n;
  }
  return nMsg;
}

// the sum over the ranks of a solver on a process grid of more than one rank: the table in the workspace, the messages of this rank, and
// the counts of MugiqHipMgSolveGridInfo
struct MgRankSum {
  const MugiqHipComm *comm = nullptr;
  const char *who = "";
  double *table = nullptr;
  std::vector<int> dim, sendEntry, recvEntry, entries;
  mutable int sums = 0;
  size_t bytes() const { return align256(sizeof(double) * (size_t)comm->size * kMgThreads); }
  void init(const MugiqHipComm *c, const char *who_) {
    comm = c, who = who_;
    const int n = rank_sum_plan(c->grid, c->coord, 0, nullptr, nullptr, nullptr, nullptr);
    dim.resize(n), sendEntry.resize(n), recvEntry.resize(n), entries.resize(n);
    rank_sum_plan(c->grid, c->coord, n, dim.data(), sendEntry.data(), recvEntry.data(), entries.data());
  }
  // every rank's entry into every rank's table, in stream order: no host read, no packing
  int gather(hipStream_t stream) const {
    for (size_t m = 0; m < dim.size(); m++)
      if (int st = comm->sendrecv(comm->ctx, table + (size_t)sendEntry[m] * kMgThreads, table + (size_t)recvEntry[m] * kMgThreads,
                                  sizeof(double) * (size_t)entries[m] * kMgThreads, dim[m], +1, stream))
        return set_error(MUGIQ_HIP_ERROR_HIP, "%s: rank sum sendrecv callback failed with status %d", who, st);
    sums++;
    return MUGIQ_HIP_SUCCESS;
  }
};

// D_i = S_i for the active i < n, from storage FS in layout Ls to storage FD in layout Ld (mg_convert_kernel)
template <typename FD, typename FS>
int mg_convert(const MgVecs<FD> &D, const MgVecs<FS> &S, const MgLayout &Ld, const MgLayout &Ls, int n, unsigned active, bool wide, hipStream_t stream) {
  const dim3 grid((unsigned)std::min<int64_t>(kMgMaxGroups, (Ls.total + kMgThreads - 1) / kMgThreads), n);
  if (!wide && Ls.total < (int64_t(1) << 31)) hipLaunchKernelGGL((mg_convert_kernel<FD, FS, uint32_t>), grid, dim3(kMgThreads), 0, stream, D, S, Ld, Ls, active);
  else hipLaunchKernelGGL((mg_convert_kernel<FD, FS, int64_t>), grid, dim3(kMgThreads), 0, stream, D, S, Ld, Ls, active);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

// one level's Krylov state in the workspace and the launches on it, for vectors stored as Cplx<F>
template <typename F> struct MgLevel {
  typedef Cplx<F> C;
  typedef MgVecs<F> Vecs;
  MgLayout L;
  int nb = 0, nGroups = 0;
  bool wide = false;  // MUGIQ_HIP_DEBUG_WIDE_INDEX, as the call found it (MgSolver::init)
  int64_t vecElems = 0;
  C *P = nullptr, *Q = nullptr;  // nDir x nb vectors each
  double *partial = nullptr, *coef = nullptr, *sc = nullptr, *res = nullptr;  // shared by all levels: the stream orders their passes (MgSolver::carve)
  hipStream_t stream = nullptr;
  const MgRankSum *rs = nullptr;  // a process grid of more than one rank: every final sum goes through the rank table

  void set(hipStream_t stream_, int nb_, bool wide_, const MgLayout &l, size_t vecBytes) {
    stream = stream_, nb = nb_, wide = wide_, L = l;
    nGroups = (int)std::min<int64_t>(kMgMaxGroups, (L.total + kMgThreads - 1) / kMgThreads);
    vecElems = (int64_t)(vecBytes / sizeof(C));
  }
  void set_scalars(unsigned char *base) {
    partial = reinterpret_cast<double *>(base);
    coef = partial + (size_t)kMgBlock * kMgMaxGroups * kMgSlots;
    sc = coef + kMgBlock * kMgSlots;
    res = sc + 4 * kMgBlock;
  }
  C *dir(C *base, int j, int v) const { return base + ((int64_t)j * nb + v) * vecElems; }
  bool narrow() const { return !wide && L.total < (int64_t(1) << 31); }
  dim3 grid(int n) const { return dim3(nGroups, n); }

  int final_sum(int nUsed, unsigned active, int mode, double omega) const {
    if (rs) {  // local sums into this rank's entry, the gather, the sum over the ranks and the epilogue of the mode
      hipLaunchKernelGGL(mg_final_sum_kernel, dim3(1), dim3(kMgThreads), 0, stream, partial, nGroups, nUsed, active, (int)kMgFinTable, omega, coef, sc, res,
                         rs->table + (size_t)rs->comm->rank * kMgThreads);
      MUGIQ_CHECK_HIP(hipGetLastError());
      if (int st = rs->gather(stream)) return st;
      hipLaunchKernelGGL(mg_rank_sum_kernel, dim3(1), dim3(kMgThreads), 0, stream, rs->table, rs->comm->size, mode, omega, coef, sc, res);
      MUGIQ_CHECK_HIP(hipGetLastError());
      return MUGIQ_HIP_SUCCESS;
    }
    hipLaunchKernelGGL(mg_final_sum_kernel, dim3(1), dim3(kMgThreads), 0, stream, partial, nGroups, nUsed, active, mode, omega, coef, sc, res,
                       (double *)nullptr);
    MUGIQ_CHECK_HIP(hipGetLastError());
    return MUGIQ_HIP_SUCCESS;
  }
#define MUGIQ_MG_LAUNCH(kernel, n, ...)                                                                                   \
  do {                                                                                                                    \
    if (narrow()) hipLaunchKernelGGL((kernel<F, uint32_t>), grid(n), dim3(kMgThreads), 0, stream, __VA_ARGS__);                \
    else hipLaunchKernelGGL((kernel<F, int64_t>), grid(n), dim3(kMgThreads), 0, stream, __VA_ARGS__);                          \
    MUGIQ_CHECK_HIP(hipGetLastError());                                                                                   \
  } while (0)

  int axpby(const Vecs &c, const Vecs *a, double sa, const Vecs *b, double sb, int n, unsigned active) const {
    const Vecs none{};
    MUGIQ_MG_LAUNCH(mg_axpby_kernel, n, c, a ? *a : none, sa, b ? *b : none, sb, L, active);
    return MUGIQ_HIP_SUCCESS;
  }
  // <t, s> and <t, t> -> mode kMgFinMr: alpha of an MR step in sc; kMgFinRaw: the sums in res
  int dot2(const Vecs &t, const Vecs &s, int n, unsigned active, int mode, double omega) const {
    MUGIQ_MG_LAUNCH(mg_dot2_kernel, n, t, s, L, active, partial);
    return final_sum(3, active, mode, omega);
  }
  int mr_update(const Vecs &z, const Vecs &s, const Vecs &t, const Vecs *sOut, bool zZero, int n, unsigned active) const {
    const Vecs none{};
    MUGIQ_MG_LAUNCH(mg_mr_update_kernel, n, z, s, t, sOut ? *sOut : none, sc, zZero ? 1 : 0, sOut ? 1 : 0, L, active);
    return MUGIQ_HIP_SUCCESS;
  }
  // step k of the GCR recurrence once q_k = A p_k is there: orthogonalise against the k stored directions, normalise, update x and r.
  // Leaves ||r||^2 of the step in res (wantNorm) for the host to fetch
  int gcr_step(int k, const Vecs &x, const Vecs &r, bool xZero, bool copyNext, bool wantNorm, int n, unsigned active) const {
    if (k > 0) {
      MUGIQ_MG_LAUNCH(mg_multidot_kernel, n, Q, vecElems, nb, k, L, active, partial);
      if (int st = final_sum(2 * k, active, kMgFinCoef, 0.0)) return st;
    }
    MUGIQ_MG_LAUNCH(mg_multiaxpy_kernel, n, P, Q, vecElems, nb, k, r, coef, L, active, partial);
    if (int st = final_sum(3, active, kMgFinNorm, 0.0)) return st;
    MUGIQ_MG_LAUNCH(mg_update_kernel, n, P, Q, vecElems, nb, k, x, r, sc, xZero ? 1 : 0, copyNext ? P : (C *)nullptr, L, active, partial);
    return wantNorm ? final_sum(1, active, kMgFinRaw, 0.0) : MUGIQ_HIP_SUCCESS;
  }
#undef MUGIQ_MG_LAUNCH
};

// which fine vectors of a block a solver keeps in the workspace
enum { kMgSetS = 1, kMgSetT = 2, kMgSetW = 4, kMgSetR = 8, kMgSetZ = 16, kMgSetsOfK = kMgSetS | kMgSetT | kMgSetW };

// the coarse levels a hierarchy may have (nCoarseLevels).  Lifting the limit is this constant and the wording of check_levels' refusal;
// it needs a reference and tests of its own first
constexpr int kMgMaxCoarse = 2;

// coarse level l >= 1 of a solver (MgSolver::coarse[l - 1]): what leads into it, its operator, and its vectors in the workspace
template <typename F> struct MgCoarse {
  const MugiqHipTransfer *transfer = nullptr;  // T_{l-1}, between level l - 1 and this one
  const MugiqHipCoarseOperator *op = nullptr;  // M_l
  MgLevel<F> lv;                               // P, Q: nDir x nb directions each
  MugiqHipCoarseField like;                    // a vector of the level, without a body
  size_t bytes = 0;                            // of one vector
  int nDir = 0;                                // stored directions: coarseIters of the cycle one level up
  bool deeper = false;                         // a level l + 1 was given: the solve here is flexible, preconditioned by the level's own cycle K_l
  MugiqHipMgSolveParam prm{};                  // the parameters of K_l (deeper only)
  MugiqHipCoarseField x[kMgBlock], r[kMgBlock];               // the solve's result and its right-hand side
  MugiqHipCoarseField s[kMgBlock], t[kMgBlock], w[kMgBlock];  // K_l's own vectors (deeper only)

  MugiqHipCoarseField dir(Cplx<F> *base, int j, int v) const {
    MugiqHipCoarseField f = like;
    f.data = lv.dir(base, j, v);
    return f;
  }
};

// the operators, the parameters and the workspace vectors of one storage F: with F = double the whole solve, or the outer iteration of
// the mixed solve; with F = float the cycle K of the mixed solve, on the sloppy fields.  The hierarchy is the caller's arrays of nGiven
// coarse levels: transfers[l] = T_l, ops[l] = M_{l+1}, params[l] = the cycle on level l (nGiven = 1: two-grid)
template <typename F> struct MgSolver {
  typedef Cplx<F> C;
  typedef MgVecs<F> Vecs;
  const MugiqHipGaugeField *gauge;
  const MugiqHipCloverField *clover;
  double kappa;
  const MugiqHipTransfer *transfers;
  const MugiqHipCoarseOperator *ops;
  const MugiqHipMgSolveParam *params;
  int nGiven;
  hipStream_t stream;
  const char *who;
  const MugiqHipCoarseDeflation *deflation;  // of the last coarse level given (NULL: none); read only where that level is in use (init)
  int nb, nDirFine, sets;
  int nCoarse;  // coarse levels in use (init): level l is, when every cycle above it takes its coarse step
  size_t fb;
  OpContext stencil;          // M of this solver: on a single domain no halo exchange and no send buffer, on a process grid (set_grid) both
  TransferSwitches switches;  // as the call found them (init)
  size_t packedBytes;         // of `packed`, the packed coarse vectors of P_0 for nb vectors (ProlongForm::workspaceBytes)
  void *packed;
  MgLevel<F> fine;
  MgCoarse<F> coarse[kMgMaxCoarse];
  // r: the solver's recursive residual (mixed solve, F = float: its rounded copy); zk: K's result before it is widened (mixed solve only)
  MugiqHipSpinorField s[kMgBlock], t[kMgBlock], w[kMgBlock], r[kMgBlock], zk[kMgBlock];
  MugiqHipSpinorField fineLike;
  bool deflated = false;     // the last-level solve is GCRdefl: a space was given and its level is in use
  size_t deflBytes = 0;      // of deflMem, the space of this call on the device (CoarseDeflationWork, csrc/mg_common.h)
  void *deflMem = nullptr;
  CoarseDeflationWork defl;
  // A rank of a process grid (set_grid, before init; the *_grid entry points, F = double, one coarse level).  part: the partitioned axes;
  // with none of them everything below is empty and the solver is the single-domain one, launch for launch
  const MugiqHipComm *comm = nullptr;
  const MugiqHipCoarseHalo *halo = nullptr;
  int part[4] = {0, 0, 0, 0};
  bool anyPart = false;
  size_t bodyBytes = 0, ghostBytes = 0, sendBytes = 0;  // of a fine vector's body and of its ghost zones (fb is their sum); of stencil.send
  unsigned char *lent[kMgBlock] = {};  // ghost zones lent to an input of the stencil that the caller owns (z of K, x of the solve)
  MgRankSum rankSum;                   // in use with more than one rank
  mutable int fineExchanges = 0;
  mutable CoarseGridCounts coarseCounts;

  void set_grid(const MugiqHipComm *comm_, const int part_[4], const MugiqHipCoarseHalo *halo_) {
    comm = comm_, halo = halo_;
    for (int d = 0; d < 4; d++) anyPart |= (part[d] = part_[d]) != 0;
  }
  void grid_info(MugiqHipMgSolveGridInfo *g) const {
    g->fineExchanges = fineExchanges, g->coarseExchanges = coarseCounts.exchanges;
    g->rankSums = rankSum.sums, g->rankSumMessages = rankSum.sums * (int)rankSum.dim.size();
  }
  // the ghost zones of f on the partitioned axes, from `zones` on (NULL: none)
  void set_ghosts(MugiqHipSpinorField &f, unsigned char *zones) const {
    for (int d = 0; d < 4; d++)
      for (int b = 0; b < 2; b++) {
        f.ghost[d][b] = part[d] && zones ? zones : nullptr;
        if (part[d] && zones) zones += stencil_zone_bytes(fineLike, (int)sizeof(F), d);
      }
  }

  static Vecs vecs(const MugiqHipSpinorField *f, int n) {
    Vecs m{};
    for (int i = 0; i < n; i++) m.p[i] = static_cast<C *>(f[i].data);
    return m;
  }
  static Vecs vecs(const MugiqHipCoarseField *f, int n) {
    Vecs m{};
    for (int i = 0; i < n; i++) m.p[i] = static_cast<C *>(f[i].data);
    return m;
  }
  MugiqHipSpinorField fine_dir(C *base, int j, int v) const {
    MugiqHipSpinorField f = fineLike;
    f.data = fine.dir(base, j, v);
    if (anyPart) set_ghosts(f, static_cast<unsigned char *>(f.data) + bodyBytes);
    return f;
  }
  template <typename T> static int gather(const T *set, int n, unsigned mask, T *out) {
    int m = 0;
    for (int i = 0; i < n; i++)
      if ((mask >> i) & 1u) out[m++] = set[i];
    return m;
  }
  // dst_i = M src_i for the active i: the batched stencil as it is.  (This, R and P: the LDS poisoned in front, where asked)
  int apply_M(const MugiqHipSpinorField *dst, const MugiqHipSpinorField *src, int n, unsigned active) const {
    MugiqHipSpinorField d[kMgBlock], sr[kMgBlock];
    const int m = gather(dst, n, active, d);
    gather(src, n, active, sr);
    if (anyPart) {  // the ghost zones of src are exchanged first; an input of the caller's that has none borrows the solver's
      for (int i = 0; i < m; i++)
        for (int dd = 0; dd < 4; dd++)
          if (part[dd] && (sr[i].ghost[dd][0] == nullptr || sr[i].ghost[dd][1] == nullptr)) {
            set_ghosts(sr[i], lent[i]);
            break;
          }
      fineExchanges++;
    }
    if (int e = debug_poison_lds_if_asked(stream)) return e;
    return stencil_apply(stencil, d, sr, m, 0, 0, 1.0);
  }
  // dst_i = A src_i for the active i, A the explicit operator of a coarse level
  int apply_coarse(const MugiqHipCoarseOperator *A, const MugiqHipCoarseField *dst, const MugiqHipCoarseField *src, int n, unsigned active) const {
    MugiqHipCoarseField d[kMgBlock], sr[kMgBlock];
    const int m = gather(dst, n, active, d);
    gather(src, n, active, sr);
    if (anyPart) return coarse_apply_grid(d, sr, m, A, halo, part, MUGIQ_HIP_EIG_OPERATOR_M, 1.0, comm, stream, false, &coarseCounts);
    return coarse_apply(d, sr, m, A, MUGIQ_HIP_EIG_OPERATOR_M, 1.0, stream);
  }
  // c_i = R f_i and f_i = P c_i through T, from and into the fine level or a coarse one: all that tells level 0 from the others in a cycle
  int restrict_to(const MugiqHipCoarseField *c, const MugiqHipSpinorField *f, int n, const MugiqHipTransfer *T) const {
    if (int e = debug_poison_lds_if_asked(stream)) return e;
    return restrict_batched(c, f, n, T, 0, stream);
  }
  int restrict_to(const MugiqHipCoarseField *c, const MugiqHipCoarseField *f, int n, const MugiqHipTransfer *T) const {
    if (int e = debug_poison_lds_if_asked(stream)) return e;
    return restrict_coarse_batched(c, f, n, T, stream);
  }
  int prolong_from(const MugiqHipSpinorField *f, const MugiqHipCoarseField *c, int n, const MugiqHipTransfer *T) const {
    if (int e = debug_poison_lds_if_asked(stream)) return e;
    return prolong_batched(f, c, n, T, switches, packed, stream);
  }
  int prolong_from(const MugiqHipCoarseField *f, const MugiqHipCoarseField *c, int n, const MugiqHipTransfer *T) const {
    if (int e = debug_poison_lds_if_asked(stream)) return e;
    return prolong_coarse_batched(f, c, n, T, stream);
  }

  // The work memory is carved from the stream's operator workspace: the scalars, the prolongator's packed coarse vectors (where a coarse
  // level is in use), then per right-hand side of a block 2 nDirFine fine
  // directions and the fine vectors of `sets` (K: s, t, w; the solver: r as well), and per coarse level in use 2 nDir directions, x and
  // r, and s, t, w of the level's own cycle where a deeper level follows (three levels: s, t, w of K_1 on level 1; level 2 only for
  // params[1].coarseIters > 0).  init() fixes the layouts and sizes (vectors laid out like `like`, stored as Cplx<F>); carve() is the one
  // statement of the layout: it places this solver's share, and run without a workspace it counts it (place()).  The mixed solve carves
  // two solvers from one reservation.  Nothing the solver calls reserves the arena again: the stencil and the transfers are the internal
  // entries, which work in what they are handed (the prolongator in `packed`), and coarse_apply with the form M takes no work memory.
  //
  // On a process grid (set_grid) two of the calls do take work memory, and the layout answers both.  The stencil packs the faces it sends
  // into OpContext::send: stencil_send_bytes for nb fields stand at the very start of this solver's share, in front of `packed`, behind the
  // rank table of more than one rank (MgRankSum; [rank][8][32] doubles, next to the scalars whose sums it completes).  coarse_apply_grid
  // keeps its send and receive faces in the stream's OTHER buffer (stream_workspace, coarse_grid_layout), which nothing else of a solve
  // uses: reserve() asks for coarse_grid_layout(M, nb).bytes there once, before the first launch, so that the reservations
  // coarse_apply_grid makes itself are no larger, move nothing and never wait for the stream (the argument of the coarse eigensolver on a
  // grid).  Every fine vector of the workspace -- the directions, s, t, w, r -- is followed by its ghost zones on the partitioned axes (fb
  // counts them; the Krylov kernels walk the body alone), since any of them may be the input of a stencil; `lent` are nb more sets of
  // zones for the inputs the caller owns.  With nothing partitioned all of these are empty and the offsets are the single-domain ones.
  void init(const MugiqHipSpinorField &like, int nDirFine_, int nVecRhs, int sets_, bool withCoarse) {
    nb = std::min(nVecRhs, kMgBlock);
    nDirFine = nDirFine_, sets = sets_;
    stencil = OpContext{gauge, comm, {part[0], part[1], part[2], part[3]}, kappa, stream, nullptr, who, clover};
    switches = transfer_switches_from_env();
    fineLike = like;
    fineLike.precision = (int)sizeof(F);
    fineLike.data = nullptr;
    for (int d = 0; d < 4; d++)
      for (int b = 0; b < 2; b++) fineLike.ghost[d][b] = nullptr;
    const bool wide = debug_wide_index_asked();
    bodyBytes = fine_bytes<F>(like);
    ghostBytes = stencil_send_bytes(like, (int)sizeof(F), part, 1);  // (one send buffer per zone: the same bytes)
    sendBytes = stencil_send_bytes(like, (int)sizeof(F), part, nb);
    fb = bodyBytes + ghostBytes;
    if (comm && comm->size > 1) rankSum.init(comm, who);
    const MgRankSum *rs = comm && comm->size > 1 ? &rankSum : nullptr;
    fine.set(stream, nb, wide, fine_layout(like), fb);
    fine.rs = rs;
    nCoarse = 0;
    for (int l = 0; l < nGiven && withCoarse && params[l].coarseIters > 0; l++) {
      MgCoarse<F> &c = coarse[nCoarse++];
      c.transfer = &transfers[l], c.op = &ops[l], c.nDir = params[l].coarseIters;
      c.deeper = l + 1 < nGiven;
      if (c.deeper) c.prm = params[l + 1];
      c.like = coarse_side_layout(*c.transfer);
      c.bytes = coarse_bytes<F>(c.like);
      c.lv.set(stream, nb, wide, coarse_layout(c.like), c.bytes);
      c.lv.rs = rs;
    }
    // (only the finest transfer has a packed form: the coarse -> coarse prolongator takes no work memory)
    deflated = deflation != nullptr && nCoarse == nGiven;
    deflBytes = deflated ? coarse_deflation_work_bytes(coarse[nCoarse - 1].like, deflation->nEv) : 0;
    packedBytes = nCoarse ? align256(select_prolong_form(transfers[0], (int)sizeof(F), like.field_order, nb, switches).workspaceBytes) : 0;
  }
  // this solver's vectors from ws + off on, ws the start of the scalars; returns the offset behind them.  ws NULL: nothing is placed,
  // the offsets are the same
  size_t carve(unsigned char *ws, size_t off) {
    // One set of scalars serves every level because the stream orders the passes and every scalar lives for one launch: a final sum
    // writes coef, (nu, alpha) or an MR alpha, and the very next launch of that level's step (multi-axpy, update, MR update) is its
    // only reader.  Nesting K_1 inside a GCR step of level 1 does not change that: p_k = K_1(r) and q_k = M_1 p_k are complete launches
    // that come BEFORE the step's own multi-dot, so no scalar of the step exists yet while K_1 and the coarsest solve overwrite them,
    // and K_1's last alpha was consumed by its last update.  Only `res` is read by the host, straight after the final sum that wrote it.
    auto take = [&](size_t bytes) {
      unsigned char *p = ws ? ws + off : nullptr;
      off += bytes;
      return p;
    };
    if (ws) fine.set_scalars(ws);
    rankSum.table = reinterpret_cast<double *>(take(rankSum.comm ? rankSum.bytes() : 0));
    stencil.send = take(sendBytes);
    for (int i = 0; i < nb; i++) lent[i] = take(ghostBytes);
    packed = take(packedBytes);
    fine.P = reinterpret_cast<C *>(take((size_t)nDirFine * nb * fb));
    fine.Q = reinterpret_cast<C *>(take((size_t)nDirFine * nb * fb));
    MugiqHipSpinorField *all[5] = {s, t, w, r, zk};
    for (int k = 0; k < 5; k++)
      for (int i = 0; i < nb && ((sets >> k) & 1); i++) {
        all[k][i] = fineLike;
        all[k][i].data = take(fb);
        if (anyPart && ws) set_ghosts(all[k][i], static_cast<unsigned char *>(all[k][i].data) + bodyBytes);
      }
    for (int l = 0; l < nCoarse; l++) {
      MgCoarse<F> &c = coarse[l];
      if (ws) c.lv.set_scalars(ws);
      c.lv.P = reinterpret_cast<C *>(take((size_t)c.nDir * nb * c.bytes));
      c.lv.Q = reinterpret_cast<C *>(take((size_t)c.nDir * nb * c.bytes));
      MugiqHipCoarseField *csets[5] = {c.x, c.r, c.s, c.t, c.w};
      for (int k = 0; k < (c.deeper ? 5 : 2); k++)
        for (int i = 0; i < nb; i++) {
          csets[k][i] = c.like;
          csets[k][i].data = take(c.bytes);
        }
    }
    // the deflation space of the call: sigma, the coefficients and the chunk partials live from one projection to the next launch that
    // reads them, across the operator applications of the recurrence -- not for one launch as the scalars above, so they get a buffer of their own
    deflMem = take(deflBytes);
    return off;
  }
  // once the workspace is placed: sigma and the body tables of the space go up, once per call
  int upload_deflation() {
    if (!deflated) return MUGIQ_HIP_SUCCESS;
    return coarse_deflation_prepare(&defl, deflation, coarse[nCoarse - 1].like, deflMem, fine.wide, stream);
  }
  // walk(ws) carves the solvers of a call behind the scalars at ws and returns the bytes it walked: once without a workspace for the
  // size of the reservation, once on it
  template <typename Walk> static int place(hipStream_t stream, const Walk &walk) {
    void *ws = nullptr;
    if (int st = stream_operator_workspace(&ws, walk(nullptr) + 256, stream)) return st;
    walk(static_cast<unsigned char *>(ws));
    return MUGIQ_HIP_SUCCESS;
  }
  // one solver alone on the workspace
  int reserve(const MugiqHipSpinorField &like, int nDirFine_, int nVecRhs, bool withR) {
    init(like, nDirFine_, nVecRhs, kMgSetsOfK | (withR ? kMgSetR : 0), true);
    if (int st = place(stream, [this](unsigned char *ws) { return carve(ws, scalar_bytes()); })) return st;
    if (anyPart && nCoarse) {  // the faces of coarse_apply_grid, once and for the most vectors a launch takes (the comment above init)
      CoarseGridLayout L;
      coarse_grid_layout(&L, coarse[0].op, part, MUGIQ_HIP_EIG_OPERATOR_M, nb);
      void *faces = nullptr;
      if (int st = stream_workspace(&faces, L.bytes, stream)) return st;
    }
    return upload_deflation();
  }

  // x = GCRfix(M_l, r, nDir) on the coarse level c for the active right-hand sides; r is used up.  With a space: GCRdefl, the same
  // recurrence started from the projection (x0, r0) of r, which takes r's place
  int gcr_fixed(const MgCoarse<F> &c, int n, unsigned active) const {
    MugiqHipCoarseField p[kMgBlock], q[kMgBlock];
    for (int i = 0; i < n; i++) p[i] = c.dir(c.lv.P, 0, i);
    const Vecs rv = vecs(c.r, n), xv = vecs(c.x, n), pv = vecs(p, n);
    if (deflated)
      if (int st = coarse_deflation_project(defl, c.x, c.r, c.r, n, active, (int)sizeof(F), stream)) return st;
    if (int st = c.lv.axpby(pv, &rv, 1.0, nullptr, 0.0, n, active)) return st;
    for (int k = 0; k < c.nDir; k++) {
      for (int i = 0; i < n; i++) {
        p[i] = c.dir(c.lv.P, k, i);
        q[i] = c.dir(c.lv.Q, k, i);
      }
      if (int st = apply_coarse(c.op, q, p, n, active)) return st;
      if (int st = c.lv.gcr_step(k, xv, rv, k == 0 && !deflated, k + 1 < c.nDir, false, n, active)) return st;
    }
    return MUGIQ_HIP_SUCCESS;
  }

  // x = the solve on level l >= 1 of r (the level's own x and r) for the active right-hand sides; r is used up.  The last level:
  // GCRfix(M_l, r, nDir).  Above it: GCRflex(M_l, K_l, r, nDir), where K_l writes its result straight into the direction slot p_k
  int solve(int l, int n, unsigned active) const {
    const MgCoarse<F> &c = coarse[l - 1];
    if (!c.deeper) return gcr_fixed(c, n, active);
    const Vecs rv = vecs(c.r, n), xv = vecs(c.x, n);
    for (int k = 0; k < c.nDir; k++) {
      MugiqHipCoarseField p[kMgBlock], q[kMgBlock];
      for (int i = 0; i < n; i++) {
        p[i] = c.dir(c.lv.P, k, i);
        q[i] = c.dir(c.lv.Q, k, i);
      }
      if (int st = cycle_on(l, p, c.r, n, active)) return st;
      if (int st = apply_coarse(c.op, q, p, n, active)) return st;
      if (int st = c.lv.gcr_step(k, xv, rv, k == 0, false, false, n, active)) return st;
    }
    return MUGIQ_HIP_SUCCESS;
  }

  // z_i = Cyc(A, R, P, S; p)(r_i) for the active i on level `lv`, with the level's own vectors s, t, w: a fixed sequence of launches,
  // nothing read back.  applyA(dst, src, n, active): dst = A src; the correction dst = P S(R src) goes through level l + 1 (correct(),
  // below) and is taken for p.coarseIters > 0 only.  z and r are not touched elsewhere; r is only read
  template <typename Fld, typename ApplyA>
  int cycle(int l, const MgLevel<F> &lv, const MugiqHipMgSolveParam &p, const ApplyA &applyA, const Fld *z, const Fld *r, const Fld *s_, const Fld *t_,
            const Fld *w_, int n, unsigned active) const {
    bool zZero = true;
    const Fld *sIn = r;  // where s lives: r itself until the first update
    const bool coarseStep = p.coarseIters > 0;
    int st;
    // one MR step on (z, sIn): t = A sIn, alpha on the device, z += alpha sIn, s = sIn - alpha t (last: s is not needed again)
    auto mr_step = [&](bool last) {
      if (int e = applyA(t_, sIn, n, active)) return e;
      const Vecs tv = vecs(t_, n), sv = vecs(sIn, n), so = vecs(s_, n);
      if (int e = lv.dot2(tv, sv, n, active, kMgFinMr, p.omega)) return e;
      const int e = lv.mr_update(vecs(z, n), sv, tv, last ? nullptr : &so, zZero, n, active);
      zZero = false;
      sIn = s_;
      return e;
    };
    for (int i = 0; i < p.nuPre; i++)
      if ((st = mr_step(!coarseStep && p.nuPost == 0 && i == p.nuPre - 1))) return st;
    if (coarseStep) {
      if ((st = correct(l, zZero ? z : w_, sIn, n, active))) return st;
      const Vecs zv = vecs(z, n), wv = vecs(w_, n);
      if (!zZero && (st = lv.axpby(zv, &zv, 1.0, &wv, 1.0, n, active))) return st;
      zZero = false;
      if (p.nuPost > 0) {  // s = r - A z, one application
        if ((st = applyA(t_, z, n, active))) return st;
        const Vecs rv = vecs(r, n), tv = vecs(t_, n);
        if ((st = lv.axpby(vecs(s_, n), &rv, 1.0, &tv, -1.0, n, active))) return st;
        sIn = s_;
      }
    }
    for (int i = 0; i < p.nuPost; i++)
      if ((st = mr_step(i == p.nuPost - 1))) return st;
    if (zZero) return lv.axpby(vecs(z, n), nullptr, 0.0, nullptr, 0.0, n, active);  // no step at all: the cycle is 0
    return MUGIQ_HIP_SUCCESS;
  }
  // d_i = P S(R src_i) for the active i, from level l through level l + 1: restrict into its r, solve there, prolong its x
  template <typename Fld> int correct(int l, const Fld *d, const Fld *src, int n, unsigned active) const {
    const MgCoarse<F> &c = coarse[l];
    Fld fa[kMgBlock];
    MugiqHipCoarseField ca[kMgBlock];
    const int na = gather(src, n, active, fa);
    gather(c.r, n, active, ca);
    if (int e = restrict_to(ca, fa, na, c.transfer)) return e;
    if (int e = solve(l + 1, n, active)) return e;
    gather(c.x, n, active, ca);
    gather(d, n, active, fa);
    return prolong_from(fa, ca, na, c.transfer);
  }

  // z_i = K_l(r_i) on the coarse level l >= 1 with a deeper one: Cyc(M_l, R_l, P_l, the solve on level l + 1; params[l])
  int cycle_on(int l, const MugiqHipCoarseField *z, const MugiqHipCoarseField *r_, int n, unsigned active) const {
    const MgCoarse<F> &c = coarse[l - 1];
    auto applyA = [&](const MugiqHipCoarseField *d, const MugiqHipCoarseField *sr, int m, unsigned act) { return apply_coarse(c.op, d, sr, m, act); };
    return cycle(l, c.lv, c.prm, applyA, z, r_, c.s, c.t, c.w, n, active);
  }
  // z_i = K(r_i) (three levels: K^(3)) for the active i: the same on level 0, Cyc(M, R_0, P_0, the solve on level 1; params[0])
  int precondition(const MugiqHipSpinorField *z, const MugiqHipSpinorField *r_, int n, unsigned active) const {
    auto applyA = [this](const MugiqHipSpinorField *d, const MugiqHipSpinorField *sr, int m, unsigned act) { return apply_M(d, sr, m, act); };
    return cycle(0, fine, params[0], applyA, z, r_, s, t, w, n, active);
  }

  // res[4 i + ..] of the last final sum, on the host: the one blocking read
  int fetch(double out[4 * kMgBlock], int *reads) const {
    MUGIQ_CHECK_HIP(hipMemcpyAsync(out, fine.res, sizeof(double) * 4 * kMgBlock, hipMemcpyDeviceToHost, stream));
    MUGIQ_CHECK_HIP(hipStreamSynchronize(stream));
    ++*reads;
    return MUGIQ_HIP_SUCCESS;
  }
};

// what a *_grid entry point adds to a call: the halo of the coarse operator, whether the input needs ghost zones, and (filled by
// check_problem) the partitioned axes
struct MgGridArgs {
  const MugiqHipCoarseHalo *halo;
  bool inNeedsGhosts;
  mutable int part[4];
};

bool same_layout(const MugiqHipSpinorField &a, const MugiqHipSpinorField &b) {
  return same_geometry(a, b) && a.stride == b.stride && a.parity_offset == b.parity_offset;
}

int check_param(const MugiqHipMgSolveParam *p, const char *who) {
  MUGIQ_REQUIRE(p != nullptr, "%s: param is NULL", who);
  MUGIQ_REQUIRE(p->tol > 0.0 && p->maxIter >= 0, "%s: tol = %g must be positive and maxIter = %d non-negative", who, p->tol, p->maxIter);
  MUGIQ_REQUIRE(p->nKrylov >= 1 && p->nKrylov <= kMgMaxDir, "%s: nKrylov = %d must be in [1, %d]", who, p->nKrylov, kMgMaxDir);
  MUGIQ_REQUIRE(p->nuPre >= 0 && p->nuPre <= 16 && p->nuPost >= 0 && p->nuPost <= 16, "%s: nuPre = %d and nuPost = %d must be in [0, 16]", who, p->nuPre,
                p->nuPost);
  MUGIQ_REQUIRE(p->coarseIters >= 0 && p->coarseIters <= kMgMaxDir, "%s: coarseIters = %d must be in [0, %d]", who, p->coarseIters, kMgMaxDir);
  MUGIQ_REQUIRE(std::isfinite(p->omega), "%s: omega = %g", who, p->omega);
  return MUGIQ_HIP_SUCCESS;
}

// everything the entry points share, before any device work: out (written) and in (read) are nVec fields of one layout and of precision
// fieldPrec, the transfer and the coarse operator of precision hierPrec.  (8, 8): the fp64 entries, which refuse anything else as
// UNSUPPORTED; (4, 4): the sloppy cycle; (8, 4): the mixed solve
int check_problem(const MugiqHipSpinorField *out, const MugiqHipSpinorField *in, int nVec, const char *outName, const char *inName,
                  const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover, const MugiqHipTransfer *transfer, const MugiqHipCoarseOperator *op,
                  const MugiqHipMgSolveParam *param, double kappa, const MugiqHipComm *comm, const char *who, int fieldPrec = 8, int hierPrec = 8,
                  const MgGridArgs *grid = nullptr) {
  MUGIQ_REQUIRE(out != nullptr && in != nullptr && transfer != nullptr && op != nullptr && gauge != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(grid == nullptr || comm != nullptr, "%s: comm is NULL (the single-domain entry points take none)", who);
  MUGIQ_REQUIRE(nVec >= 1, "%s: nVec = %d must be >= 1", who, nVec);
  int st;
  if ((st = check_param(param, who))) return st;
  int part[4] = {0, 0, 0, 0};
  if (grid) {  // comm -> part, the operator, and its halo on every partitioned axis
    if ((st = check_coarse_grid(comm, op, grid->halo, part, false, who))) return st;
    for (int d = 0; d < 4; d++) grid->part[d] = part[d];
    // the rank table has comm->size entries and the plan addresses it through grid and coord: they must describe one grid
    long long ranks = 1, me = 0;
    for (int d = 0; d < 4; d++) {
      MUGIQ_REQUIRE(comm->grid[d] >= 1 && comm->coord[d] >= 0 && comm->coord[d] < comm->grid[d], "%s: comm grid[%d] = %d, coord[%d] = %d", who, d,
                    comm->grid[d], d, comm->coord[d]);
      ranks *= comm->grid[d];
      me = me * comm->grid[d] + comm->coord[d];
    }
    MUGIQ_REQUIRE(ranks == comm->size && me == comm->rank, "%s: comm grid %d x %d x %d x %d and rank %d do not match size %d (x slowest, t fastest)", who,
                  comm->grid[0], comm->grid[1], comm->grid[2], comm->grid[3], comm->rank, comm->size);
  } else {
    if ((st = check_single_domain(comm, who))) return st;
    if ((st = validate_coarse_operator(op, who))) return st;
  }
  MUGIQ_REQUIRE(transfer->V != nullptr, "%s: transfer / null vectors are NULL", who);
  for (int i = 0; i < nVec; i++) {
    if ((st = validate_spinor(&out[i], who, outName))) return st;
    if ((st = validate_spinor(&in[i], who, inName))) return st;
  }
  if (fieldPrec == 8 && hierPrec == 8) {
    if (transfer->precision != 8 || op->precision != 8 || out[0].precision != 8 || in[0].precision != 8)
      return set_error(MUGIQ_HIP_ERROR_UNSUPPORTED, "%s: fp64 only: the transfer has precision %d, the coarse operator %d, %s %d and %s %d", who,
                       transfer->precision, op->precision, outName, out[0].precision, inName, in[0].precision);
  } else if (fieldPrec == 4) {
    MUGIQ_REQUIRE(transfer->precision == 4 && op->precision == 4 && out[0].precision == 4 && in[0].precision == 4,
                  "%s: fp32 storage only (mugiq_hip_mg_precondition serves precision 8): the transfer has precision %d, the coarse operator %d, %s %d and %s %d",
                  who, transfer->precision, op->precision, outName, out[0].precision, inName, in[0].precision);
  } else {
    MUGIQ_REQUIRE(transfer->precision == 4 && op->precision == 4 && out[0].precision == 8 && in[0].precision == 8,
                  "%s: %s and %s are fp64 and the sloppy hierarchy is fp32 (mugiq_hip_mg_solve serves an fp64 hierarchy): the sloppy transfer has precision %d, "
                  "the sloppy coarse operator %d, %s %d and %s %d",
                  who, outName, inName, transfer->precision, op->precision, outName, out[0].precision, inName, in[0].precision);
  }
  for (int i = 0; i < nVec; i++)
    MUGIQ_REQUIRE(same_layout(out[i], out[0]) && same_layout(in[i], out[0]),
                  "%s: vector %d of %s or %s differs in precision, field order, geometry, stride or parity offset from %s vector 0", who, i, outName, inName,
                  outName);
  if ((st = validate_transfer_operator(transfer, op, who))) return st;  // (the precisions agree by the checks above)
  for (int d = 0; d < 4; d++)
    MUGIQ_REQUIRE(in[0].X[d] == transfer->X[d], "%s: the fields have X[%d] = %d, the transfer %d", who, d, in[0].X[d], transfer->X[d]);
  if ((st = check_gauge(gauge, in[0].X, part, who))) return st;
  if (clover) {
    if ((st = validate_clover(clover, in[0].X, in[0].volumeCB, who))) return st;
    MUGIQ_REQUIRE(clover->precision == gauge->precision, "%s: clover precision %d differs from the gauge precision %d", who, clover->precision, gauge->precision);
  }
  // an input of the stencil that the caller owns and the solver does not copy (r of the cycle) brings its ghost zones
  for (int d = 0; grid && grid->inNeedsGhosts && d < 4; d++)
    for (int i = 0; part[d] && i < nVec; i++)
      MUGIQ_REQUIRE(in[i].ghost[d][0] != nullptr && in[i].ghost[d][1] != nullptr, "%s: dimension %d is partitioned but %s vector %d has no ghost zones for it",
                    who, d, inName, i);
  // the operator must be the one of this M: a coarse operator of another kappa or clover term would still converge, only slowly and silently
  MUGIQ_REQUIRE(op->kappa == kappa, "%s: the coarse operator was built for kappa = %.17g, the call has kappa = %.17g", who, op->kappa, kappa);
  MUGIQ_REQUIRE((op->hasClover != 0) == (clover != nullptr), "%s: the coarse operator was built %s a clover field, the call is %s one", who,
                op->hasClover ? "with" : "without", clover ? "with" : "without");
  if ((st = check_disjoint(out, nVec, outName, nullptr, 0, outName, who))) return st;
  return check_disjoint(out, nVec, outName, in, nVec, inName, who);
}

// check_problem for a hierarchy of L = nCoarseLevels coarse levels: level 0 as above with params_h[0]; for every l >= 1 also
// T_l = transfers_h[l] (a coarse -> coarse transfer on the lattice and with the colours of M_l), M_{l+1} = coarseOps_h[l] (on its coarse
// side) and params_h[l].  Everything before any device work; a NULL array is refused by check_problem, which sees its element 0
int check_levels(const MugiqHipSpinorField *out, const MugiqHipSpinorField *in, int nVec, const char *outName, const char *inName,
                 const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover, const MugiqHipTransfer *transfers_h, const MugiqHipCoarseOperator *coarseOps_h,
                 int nCoarseLevels, const MugiqHipMgSolveParam *params_h, double kappa, const MugiqHipComm *comm, const char *who, int fieldPrec = 8,
                 int hierPrec = 8, const MgGridArgs *grid = nullptr) {
  static_assert(kMgMaxCoarse == 2, "the message below names the cycles that exist");
  if (nCoarseLevels < 1 || nCoarseLevels > kMgMaxCoarse)
    return set_error(MUGIQ_HIP_ERROR_UNSUPPORTED, "%s: nCoarseLevels = %d: a two-grid (1) or a three-level (2) cycle", who, nCoarseLevels);
  int st;
  if ((st = check_problem(out, in, nVec, outName, inName, gauge, clover, transfers_h, coarseOps_h, params_h, kappa, comm, who, fieldPrec, hierPrec, grid))) return st;
  for (int l = 1; l < nCoarseLevels; l++) {
    const MugiqHipTransfer *T = &transfers_h[l];
    const MugiqHipCoarseOperator *Ma = &coarseOps_h[l - 1], *Mb = &coarseOps_h[l];  // M_l above the transfer, M_{l+1} below it
    const MugiqHipMgSolveParam *p = &params_h[l];
    if ((st = check_param(p, who))) return st;
    MUGIQ_REQUIRE(p->nuPre + p->nuPost + p->coarseIters > 0, "%s: params[%d] has nuPre = nuPost = coarseIters = 0: the level-%d cycle would be zero", who, l, l);
    if ((st = validate_coarse_operator(Mb, who))) return st;
    MUGIQ_REQUIRE(T->V != nullptr, "%s: transfer %d / null vectors are NULL", who, l);
    if (T->precision != hierPrec || Mb->precision != hierPrec)
      return set_error(fieldPrec == 8 && hierPrec == 8 ? MUGIQ_HIP_ERROR_UNSUPPORTED : MUGIQ_HIP_ERROR_INVALID_ARGUMENT,
                       "%s: one precision per hierarchy: transfer 0 has precision %d, transfer %d %d and coarse operator %d %d", who, hierPrec, l, T->precision, l,
                       Mb->precision);
    for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(T->X[d] > 0 && T->geoBlockSize[d] >= 1, "%s: transfer %d: X / geo_block_size[%d]", who, l, d);
    MugiqHipCoarseField above = coarse_side_layout(transfers_h[l - 1]), below = coarse_side_layout(*T);
    above.data = reinterpret_cast<void *>(uintptr_t(16));  // geometry only: the validator wants distinct non-NULL bodies and never reads them
    below.data = reinterpret_cast<void *>(uintptr_t(32));
    if ((st = validate_coarse_transfer(T, &above, &below, 1, who))) return st;  // spin_block_size 1, on the lattice of M_l, even coarsest dims
    MUGIQ_REQUIRE(T->parity_offset == (int64_t)2 * Ma->nVec * T->nVec * T->stride,
                  "%s: transfer %d must have parity_offset = 2 nColor n_vec stride with the nColor = %d of coarse operator %d, not %lld", who, l, Ma->nVec, l - 1,
                  (long long)T->parity_offset);
    MUGIQ_REQUIRE(Mb->nVec == T->nVec, "%s: coarse operator %d has n_vec %d, transfer %d %d", who, l, Mb->nVec, l, T->nVec);
    for (int d = 0; d < 4; d++)
      MUGIQ_REQUIRE(Mb->X[d] == below.X[d], "%s: coarse operator %d X[%d] = %d, the coarse lattice of transfer %d has %d", who, l, d, Mb->X[d], l, below.X[d]);
    MUGIQ_REQUIRE(Mb->kappa == kappa, "%s: coarse operator %d was built for kappa = %.17g, the call has kappa = %.17g", who, l, Mb->kappa, kappa);
    MUGIQ_REQUIRE((Mb->hasClover != 0) == (clover != nullptr), "%s: coarse operator %d was built %s a clover field, the call is %s one", who, l,
                  Mb->hasClover ? "with" : "without", clover ? "with" : "without");
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(Ma->data), a1 = a0 + mugiq_hip_coarse_operator_bytes(Ma->X, Ma->nVec, Ma->precision);
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(Mb->data), b1 = b0 + mugiq_hip_coarse_operator_bytes(Mb->X, Mb->nVec, Mb->precision);
    MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1), "%s: coarse operator %d overlaps coarse operator %d", who, l, l - 1);
  }
  return MUGIQ_HIP_SUCCESS;
}

// the space of a *_deflated call (NULL: none, nothing to check) against the last operator of the hierarchy check_levels admitted and the
// call's own fields, before any device work
int check_deflation(const MugiqHipCoarseDeflation *d, const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels, const MugiqHipSpinorField *out,
                    const MugiqHipSpinorField *in, int nVec, const char *who) {
  if (d == nullptr) return MUGIQ_HIP_SUCCESS;
  std::vector<uintptr_t> span(4 * (size_t)nVec);
  uintptr_t(*fields)[2] = reinterpret_cast<uintptr_t(*)[2]>(span.data());
  for (int i = 0; i < nVec; i++) {
    spinor_span(out[i], &fields[i][0], &fields[i][1]);
    spinor_span(in[i], &fields[nVec + i][0], &fields[nVec + i][1]);
  }
  return check_coarse_deflation(d, &coarseOps_h[nCoarseLevels - 1], fields, 2 * nVec, who);
}

// The outer flexible GCR of mugiq_hip_mg_solve on the vectors of S (fp64).  K32 NULL: p = K(r) is S's own cycle; otherwise the cycle of
// K32 in fp32 storage, between two conversions.  Everything else -- operator applications, directions, residual, tol, the history and the
// true residual -- is the same code for both
int outer_solve(MgSolver<double> &S, const MgSolver<float> *K32, const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec,
                const MugiqHipMgSolveParam *param, int *iters_out, double *relres_out, double *history_out, int historyStride, int *hostReads_out,
                const char *who) {
  const int nK = param->nKrylov;
  int st;
  const MugiqHipSpinorField *r = S.r;
  const double tol2 = param->tol * param->tol;
  bool allConverged = true;
  int reads = 0;
  double sums[4 * kMgBlock];
  for (int v0 = 0; v0 < nVec; v0 += kMgBlock) {
    const int n = std::min(kMgBlock, nVec - v0);
    const unsigned all = (1u << n) - 1u;
    const MugiqHipSpinorField *x = x_h + v0, *b = b_h + v0;
    const MgVecs<double> xv = MgSolver<double>::vecs(x, n), bv = MgSolver<double>::vecs(b, n), rv = MgSolver<double>::vecs(r, n);
    double bn2[kMgBlock], rr[kMgBlock];
    // x = 0, r = b, ||b||^2
    if ((st = S.fine.axpby(xv, nullptr, 0.0, nullptr, 0.0, n, all))) return st;
    if ((st = S.fine.axpby(rv, &bv, 1.0, nullptr, 0.0, n, all))) return st;
    if ((st = S.fine.dot2(bv, bv, n, all, kMgFinRaw, 0.0))) return st;
    if ((st = S.fetch(sums, &reads))) return st;
    unsigned active = 0;
    for (int i = 0; i < n; i++) {
      bn2[i] = rr[i] = sums[4 * i + 2];
      iters_out[v0 + i] = 0;
      if (bn2[i] > 0.0 && !(rr[i] <= tol2 * bn2[i])) active |= 1u << i;
    }
    int k = 0;
    for (int it = 0; it < param->maxIter && active; it++) {
      MugiqHipSpinorField p[kMgBlock], q[kMgBlock];
      for (int i = 0; i < n; i++) {
        p[i] = S.fine_dir(S.fine.P, k, i);
        q[i] = S.fine_dir(S.fine.Q, k, i);
      }
      if (K32) {
        // p = K(r) with the cycle in fp32 storage: r rounded to fp32, K, z widened straight into the direction slot.  No scaling of r
        // is needed: K is homogeneous, and a residual of 1e-10 ||b|| is far inside fp32's exponent range (2^-126 = 1e-38)
        const MgVecs<float> r32 = MgSolver<float>::vecs(K32->r, n), z32 = MgSolver<float>::vecs(K32->zk, n);
        if ((st = mg_convert(r32, rv, K32->fine.L, S.fine.L, n, active, S.fine.wide, S.stream))) return st;
        if ((st = K32->precondition(K32->zk, K32->r, n, active))) return st;
        if ((st = mg_convert(MgSolver<double>::vecs(p, n), z32, S.fine.L, K32->fine.L, n, active, S.fine.wide, S.stream))) return st;
      } else if ((st = S.precondition(p, r, n, active))) {
        return st;
      }
      if ((st = S.apply_M(q, p, n, active))) return st;
      if ((st = S.fine.gcr_step(k, xv, rv, false, false, true, n, active))) return st;
      if ((st = S.fetch(sums, &reads))) return st;
      unsigned next = active;
      for (int i = 0; i < n; i++) {
        if (!((active >> i) & 1u)) continue;
        rr[i] = sums[4 * i];
        if (history_out) history_out[(size_t)(v0 + i) * historyStride + iters_out[v0 + i]] = std::sqrt(rr[i] / bn2[i]);
        iters_out[v0 + i]++;
        if (rr[i] <= tol2 * bn2[i]) next &= ~(1u << i);
      }
      active = next;
      if (++k == nK) k = 0;  // restart: the directions are cleared
    }
    // the true residual ||b - M x|| / ||b||, with one more application
    if ((st = S.apply_M(S.t, x, n, all))) return st;
    const MgVecs<double> tv = MgSolver<double>::vecs(S.t, n);
    if ((st = S.fine.axpby(tv, &bv, 1.0, &tv, -1.0, n, all))) return st;
    if ((st = S.fine.dot2(tv, tv, n, all, kMgFinRaw, 0.0))) return st;
    if ((st = S.fetch(sums, &reads))) return st;
    for (int i = 0; i < n; i++) {
      relres_out[v0 + i] = bn2[i] > 0.0 ? std::sqrt(sums[4 * i + 2] / bn2[i]) : 0.0;
      if (bn2[i] > 0.0 && !(rr[i] <= tol2 * bn2[i])) allConverged = false;
    }
  }
  if (hostReads_out) *hostReads_out = reads;
  if (!allConverged)
    return set_error(MUGIQ_HIP_ERROR_NOT_CONVERGED,
                     "%s: not every right-hand side reached tol = %g within maxIter = %d (x, iters_out, relres_out and history_out are filled)", who, param->tol,
                     param->maxIter);
  return MUGIQ_HIP_SUCCESS;
}

// the four entry points, for either number of levels; `who` names the caller in every message
template <typename F>
int precondition_levels(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover,
                        double kappa, const MugiqHipTransfer *transfers_h, const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels,
                        const MugiqHipMgSolveParam *params_h, const MugiqHipCoarseDeflation *deflation, const MugiqHipComm *comm, void *stream,
                        const char *who, const MgGridArgs *grid = nullptr) {
  const int prec = (int)sizeof(F);
  int st;
  if ((st = check_levels(z_h, r_h, nVec, "z", "r", gauge, clover, transfers_h, coarseOps_h, nCoarseLevels, params_h, kappa, comm, who, prec, prec, grid)))
    return st;
  if ((st = check_deflation(deflation, coarseOps_h, nCoarseLevels, z_h, r_h, nVec, who))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  MgSolver<F> S{gauge, clover, kappa, transfers_h, coarseOps_h, params_h, nCoarseLevels, s, who, deflation};
  if (grid) S.set_grid(comm, grid->part, grid->halo);
  if ((st = S.reserve(r_h[0], 0, nVec, false))) return st;
  for (int v0 = 0; v0 < nVec; v0 += kMgBlock) {
    const int n = std::min(kMgBlock, nVec - v0);
    if ((st = S.precondition(z_h + v0, r_h + v0, n, (1u << n) - 1u))) return st;
  }
  return MUGIQ_HIP_SUCCESS;
}

int solve_levels(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover,
                 double kappa, const MugiqHipTransfer *transfers_h, const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels,
                 const MugiqHipMgSolveParam *params_h, const MugiqHipCoarseDeflation *deflation, int *iters_out, double *relres_out, double *history_out,
                 int historyStride, int *hostReads_out, const MugiqHipComm *comm, void *stream, const char *who, const MgGridArgs *grid = nullptr,
                 MugiqHipMgSolveGridInfo *gridInfo_out = nullptr) {
  MUGIQ_REQUIRE(iters_out != nullptr && relres_out != nullptr && (grid == nullptr || gridInfo_out != nullptr), "%s: NULL argument", who);
  int st;
  if ((st = check_levels(x_h, b_h, nVec, "x", "b", gauge, clover, transfers_h, coarseOps_h, nCoarseLevels, params_h, kappa, comm, who, 8, 8, grid))) return st;
  if ((st = check_deflation(deflation, coarseOps_h, nCoarseLevels, x_h, b_h, nVec, who))) return st;
  const MugiqHipMgSolveParam *param = &params_h[0];
  MUGIQ_REQUIRE(history_out == nullptr || historyStride >= param->maxIter, "%s: historyStride = %d is smaller than maxIter = %d", who, historyStride,
                param->maxIter);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  MgSolver<double> S{gauge, clover, kappa, transfers_h, coarseOps_h, params_h, nCoarseLevels, s, who, deflation};
  if (grid) S.set_grid(comm, grid->part, grid->halo);
  if ((st = S.reserve(b_h[0], param->nKrylov, nVec, true))) return st;
  st = outer_solve(S, nullptr, x_h, b_h, nVec, param, iters_out, relres_out, history_out, historyStride, hostReads_out, who);
  if (gridInfo_out && (st == MUGIQ_HIP_SUCCESS || st == MUGIQ_HIP_ERROR_NOT_CONVERGED)) S.grid_info(gridInfo_out);
  return st;
}

int solve_mixed_levels(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                       const MugiqHipCloverField *clover, double kappa, const MugiqHipGaugeField *gaugeSloppy, const MugiqHipCloverField *cloverSloppy,
                       const MugiqHipTransfer *transfersSloppy_h, const MugiqHipCoarseOperator *coarseOpsSloppy_h, int nCoarseLevels,
                       const MugiqHipMgSolveParam *params_h, const MugiqHipCoarseDeflation *deflation, int *iters_out, double *relres_out,
                       double *history_out, int historyStride, int *hostReads_out, const MugiqHipComm *comm, void *stream, const char *who) {
  MUGIQ_REQUIRE(iters_out != nullptr && relres_out != nullptr, "%s: NULL argument", who);
  int st;
  if ((st = check_levels(x_h, b_h, nVec, "x", "b", gauge, clover, transfersSloppy_h, coarseOpsSloppy_h, nCoarseLevels, params_h, kappa, comm, who, 8, 4)))
    return st;
  if ((st = check_deflation(deflation, coarseOpsSloppy_h, nCoarseLevels, x_h, b_h, nVec, who))) return st;
  const MugiqHipMgSolveParam *param = &params_h[0];
  MUGIQ_REQUIRE(history_out == nullptr || historyStride >= param->maxIter, "%s: historyStride = %d is smaller than maxIter = %d", who, historyStride,
                param->maxIter);
  // the cycle's own fields: both or neither where the operator has a clover term; without one only gaugeSloppy can be given
  MUGIQ_REQUIRE(!(cloverSloppy != nullptr && gaugeSloppy == nullptr), "%s: cloverSloppy without gaugeSloppy (give both, or neither to use gauge and clover)", who);
  MUGIQ_REQUIRE(!(gaugeSloppy != nullptr && (cloverSloppy != nullptr) != (clover != nullptr)),
                "%s: gaugeSloppy %s cloverSloppy, but the call is %s a clover field (give both, or neither to use gauge and clover)", who,
                cloverSloppy ? "with" : "without", clover ? "with" : "without");
  if (gaugeSloppy) {
    const int part[4] = {0, 0, 0, 0};
    if ((st = check_gauge(gaugeSloppy, b_h[0].X, part, who))) return st;
    if (cloverSloppy) {
      if ((st = validate_clover(cloverSloppy, b_h[0].X, b_h[0].volumeCB, who))) return st;
      MUGIQ_REQUIRE(cloverSloppy->precision == gaugeSloppy->precision, "%s: cloverSloppy precision %d differs from the gaugeSloppy precision %d", who,
                    cloverSloppy->precision, gaugeSloppy->precision);
    }
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  // the outer iteration: 2 nKrylov directions, r and t (for the true residual) in fp64; the cycle: r and z rounded, s, t, w and the coarse
  // levels in fp32.  One reservation, the scalars shared: the stream orders every pass
  MgSolver<double> S{gauge, clover, kappa, transfersSloppy_h, coarseOpsSloppy_h, params_h, nCoarseLevels, s, who, nullptr};
  MgSolver<float> K{gaugeSloppy ? gaugeSloppy : gauge, gaugeSloppy ? cloverSloppy : clover, kappa, transfersSloppy_h, coarseOpsSloppy_h, params_h, nCoarseLevels, s, who,
                    deflation};
  S.init(b_h[0], param->nKrylov, nVec, kMgSetT | kMgSetR, false);
  K.init(b_h[0], 0, nVec, kMgSetsOfK | kMgSetR | kMgSetZ, true);
  if ((st = MgSolver<double>::place(s, [&](unsigned char *ws) { return K.carve(ws, S.carve(ws, scalar_bytes())); }))) return st;
  if ((st = K.upload_deflation())) return st;
  return outer_solve(S, &K, x_h, b_h, nVec, param, iters_out, relres_out, history_out, historyStride, hostReads_out, who);
}

}  // namespace
}  // namespace mugiq

using namespace mugiq;

extern "C" {

int mugiq_hip_mg_solve_param_default(MugiqHipMgSolveParam *param) {
  MUGIQ_REQUIRE(param != nullptr, "mgSolveParamDefault: param is NULL");
  param->tol = 1e-10;
  param->maxIter = 1000;
  param->nKrylov = 16;
  param->nuPre = 0;
  param->nuPost = 4;
  param->omega = 1.0;
  param->coarseIters = 8;
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_mg_precondition(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                              const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfer, const MugiqHipCoarseOperator *coarseOp,
                              const MugiqHipMgSolveParam *param, const MugiqHipComm *comm, void *stream) {
  return precondition_levels<double>(z_h, r_h, nVec, gauge, clover, kappa, transfer, coarseOp, 1, param, nullptr, comm, stream, "mgPrecondition");
}

int mugiq_hip_mg_solve(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                       const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfer, const MugiqHipCoarseOperator *coarseOp,
                       const MugiqHipMgSolveParam *param, int *iters_out, double *relres_out, double *history_out, int historyStride, int *hostReads_out,
                       const MugiqHipComm *comm, void *stream) {
  return solve_levels(x_h, b_h, nVec, gauge, clover, kappa, transfer, coarseOp, 1, param, nullptr, iters_out, relres_out, history_out, historyStride, hostReads_out,
                      comm, stream, "mgSolve");
}

/* the two-grid fp64 cycle and solve for a rank of a process grid.  With nothing partitioned the launches of the two calls above */
int mugiq_hip_mg_precondition_grid(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                                   const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfer, const MugiqHipCoarseOperator *coarseOp,
                                   const MugiqHipCoarseHalo *halo, const MugiqHipMgSolveParam *param, const MugiqHipComm *comm, void *stream) {
  const MgGridArgs grid{halo, true, {0, 0, 0, 0}};
  return precondition_levels<double>(z_h, r_h, nVec, gauge, clover, kappa, transfer, coarseOp, 1, param, nullptr, comm, stream, "mgPreconditionGrid", &grid);
}

int mugiq_hip_mg_solve_grid(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                            const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfer, const MugiqHipCoarseOperator *coarseOp,
                            const MugiqHipCoarseHalo *halo, const MugiqHipMgSolveParam *param, int *iters_out, double *relres_out, double *history_out,
                            int historyStride, int *hostReads_out, MugiqHipMgSolveGridInfo *gridInfo_out, const MugiqHipComm *comm, void *stream) {
  const MgGridArgs grid{halo, false, {0, 0, 0, 0}};
  return solve_levels(x_h, b_h, nVec, gauge, clover, kappa, transfer, coarseOp, 1, param, nullptr, iters_out, relres_out, history_out, historyStride, hostReads_out,
                      comm, stream, "mgSolveGrid", &grid, gridInfo_out);
}

int mugiq_hip_mg_rank_sum_plan(const int grid[4], const int coord[4], int maxOps, int *dim_out, int *sendEntry_out, int *recvEntry_out, int *entries_out) {
  if (grid == nullptr || coord == nullptr || maxOps < 0) return -1;
  for (int d = 0; d < 4; d++)
    if (grid[d] < 1 || coord[d] < 0 || coord[d] >= grid[d]) return -1;
  return rank_sum_plan(grid, coord, maxOps, dim_out, sendEntry_out, recvEntry_out, entries_out);
}

int mugiq_hip_mg_precondition_sloppy(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                                     const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfer,
                                     const MugiqHipCoarseOperator *coarseOp, const MugiqHipMgSolveParam *param, const MugiqHipComm *comm, void *stream) {
  return precondition_levels<float>(z_h, r_h, nVec, gauge, clover, kappa, transfer, coarseOp, 1, param, nullptr, comm, stream, "mgPreconditionSloppy");
}

int mugiq_hip_mg_solve_mixed(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                             const MugiqHipCloverField *clover, double kappa, const MugiqHipGaugeField *gaugeSloppy,
                             const MugiqHipCloverField *cloverSloppy, const MugiqHipTransfer *transferSloppy, const MugiqHipCoarseOperator *coarseOpSloppy,
                             const MugiqHipMgSolveParam *param, int *iters_out, double *relres_out, double *history_out, int historyStride,
                             int *hostReads_out, const MugiqHipComm *comm, void *stream) {
  return solve_mixed_levels(x_h, b_h, nVec, gauge, clover, kappa, gaugeSloppy, cloverSloppy, transferSloppy, coarseOpSloppy, 1, param, nullptr, iters_out, relres_out,
                            history_out, historyStride, hostReads_out, comm, stream, "mgSolveMixed");
}

int mugiq_hip_mg_precondition_levels(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                                     const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfers_h,
                                     const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                     const MugiqHipComm *comm, void *stream) {
  return precondition_levels<double>(z_h, r_h, nVec, gauge, clover, kappa, transfers_h, coarseOps_h, nCoarseLevels, params_h, nullptr, comm, stream,
                                     "mgPrecondition(levels)");
}

int mugiq_hip_mg_solve_levels(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                              const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfers_h, const MugiqHipCoarseOperator *coarseOps_h,
                              int nCoarseLevels, const MugiqHipMgSolveParam *params_h, int *iters_out, double *relres_out, double *history_out,
                              int historyStride, int *hostReads_out, const MugiqHipComm *comm, void *stream) {
  return solve_levels(x_h, b_h, nVec, gauge, clover, kappa, transfers_h, coarseOps_h, nCoarseLevels, params_h, nullptr, iters_out, relres_out, history_out,
                      historyStride, hostReads_out, comm, stream, "mgSolve(levels)");
}

int mugiq_hip_mg_precondition_sloppy_levels(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                                            const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfers_h,
                                            const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                            const MugiqHipComm *comm, void *stream) {
  return precondition_levels<float>(z_h, r_h, nVec, gauge, clover, kappa, transfers_h, coarseOps_h, nCoarseLevels, params_h, nullptr, comm, stream,
                                    "mgPreconditionSloppy(levels)");
}

int mugiq_hip_mg_solve_mixed_levels(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                                    const MugiqHipCloverField *clover, double kappa, const MugiqHipGaugeField *gaugeSloppy,
                                    const MugiqHipCloverField *cloverSloppy, const MugiqHipTransfer *transfersSloppy_h,
                                    const MugiqHipCoarseOperator *coarseOpsSloppy_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h, int *iters_out,
                                    double *relres_out, double *history_out, int historyStride, int *hostReads_out, const MugiqHipComm *comm, void *stream) {
  return solve_mixed_levels(x_h, b_h, nVec, gauge, clover, kappa, gaugeSloppy, cloverSloppy, transfersSloppy_h, coarseOpsSloppy_h, nCoarseLevels, params_h,
                            nullptr, iters_out, relres_out, history_out, historyStride, hostReads_out, comm, stream, "mgSolveMixed(levels)");
}

/* the *_levels entry points with a deflation space for the last coarse level (NULL: the twin) */
int mugiq_hip_mg_precondition_levels_deflated(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                                              const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfers_h,
                                              const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                              const MugiqHipCoarseDeflation *deflation, const MugiqHipComm *comm, void *stream) {
  return precondition_levels<double>(z_h, r_h, nVec, gauge, clover, kappa, transfers_h, coarseOps_h, nCoarseLevels, params_h, deflation, comm, stream,
                                     "mgPrecondition(levels, deflated)");
}

int mugiq_hip_mg_solve_levels_deflated(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                                       const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfers_h,
                                       const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                       const MugiqHipCoarseDeflation *deflation, int *iters_out, double *relres_out, double *history_out,
                                       int historyStride, int *hostReads_out, const MugiqHipComm *comm, void *stream) {
  return solve_levels(x_h, b_h, nVec, gauge, clover, kappa, transfers_h, coarseOps_h, nCoarseLevels, params_h, deflation, iters_out, relres_out, history_out,
                      historyStride, hostReads_out, comm, stream, "mgSolve(levels, deflated)");
}

int mugiq_hip_mg_precondition_sloppy_levels_deflated(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec,
                                                     const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover, double kappa,
                                                     const MugiqHipTransfer *transfers_h, const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels,
                                                     const MugiqHipMgSolveParam *params_h, const MugiqHipCoarseDeflation *deflation,
                                                     const MugiqHipComm *comm, void *stream) {
  return precondition_levels<float>(z_h, r_h, nVec, gauge, clover, kappa, transfers_h, coarseOps_h, nCoarseLevels, params_h, deflation, comm, stream,
                                    "mgPreconditionSloppy(levels, deflated)");
}

int mugiq_hip_mg_solve_mixed_levels_deflated(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                                             const MugiqHipCloverField *clover, double kappa, const MugiqHipGaugeField *gaugeSloppy,
                                             const MugiqHipCloverField *cloverSloppy, const MugiqHipTransfer *transfersSloppy_h,
                                             const MugiqHipCoarseOperator *coarseOpsSloppy_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                             const MugiqHipCoarseDeflation *deflation, int *iters_out, double *relres_out, double *history_out,
                                             int historyStride, int *hostReads_out, const MugiqHipComm *comm, void *stream) {
  return solve_mixed_levels(x_h, b_h, nVec, gauge, clover, kappa, gaugeSloppy, cloverSloppy, transfersSloppy_h, coarseOpsSloppy_h, nCoarseLevels, params_h,
                            deflation, iters_out, relres_out, history_out, historyStride, hostReads_out, comm, stream, "mgSolveMixed(levels, deflated)");
}

/* dst_i = src_i between two precisions: fields of one geometry and field order, each set with its own stride and parity offset */
int mugiq_hip_mg_convert_precision(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec, void *stream) {
  const char *who = "mgConvertPrecision";
  MUGIQ_REQUIRE(dst_h != nullptr && src_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nVec >= 1, "%s: nVec = %d must be >= 1", who, nVec);
  int st;
  for (int i = 0; i < nVec; i++) {
    if ((st = validate_spinor(&dst_h[i], who, "dst"))) return st;
    if ((st = validate_spinor(&src_h[i], who, "src"))) return st;
    MUGIQ_REQUIRE(same_layout(dst_h[i], dst_h[0]) && same_layout(src_h[i], src_h[0]), "%s: vector %d differs from vector 0 of its set", who, i);
  }
  MUGIQ_REQUIRE(dst_h[0].field_order == src_h[0].field_order && dst_h[0].volumeCB == src_h[0].volumeCB && dst_h[0].nParity == src_h[0].nParity,
                "%s: dst and src differ in field order or geometry", who);
  for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(dst_h[0].X[d] == src_h[0].X[d], "%s: dst X[%d] = %d, src %d", who, d, dst_h[0].X[d], src_h[0].X[d]);
  if ((st = check_disjoint(dst_h, nVec, "dst", src_h, nVec, "src", who))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const MgLayout Ld = fine_layout(dst_h[0]), Ls = fine_layout(src_h[0]);
  const bool wide = debug_wide_index_asked();
  const int pd = dst_h[0].precision, ps = src_h[0].precision;
  for (int v0 = 0; v0 < nVec; v0 += kMgBlock) {
    const int n = std::min(kMgBlock, nVec - v0);
    const unsigned all = (1u << n) - 1u;
    if (pd == 4 && ps == 8) st = mg_convert(MgSolver<float>::vecs(dst_h + v0, n), MgSolver<double>::vecs(src_h + v0, n), Ld, Ls, n, all, wide, s);
    else if (pd == 8 && ps == 4) st = mg_convert(MgSolver<double>::vecs(dst_h + v0, n), MgSolver<float>::vecs(src_h + v0, n), Ld, Ls, n, all, wide, s);
    else if (pd == 8) st = mg_convert(MgSolver<double>::vecs(dst_h + v0, n), MgSolver<double>::vecs(src_h + v0, n), Ld, Ls, n, all, wide, s);
    else st = mg_convert(MgSolver<float>::vecs(dst_h + v0, n), MgSolver<float>::vecs(src_h + v0, n), Ld, Ls, n, all, wide, s);
    if (st) return st;
  }
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_transfer_convert(const MugiqHipTransfer *dst, const MugiqHipTransfer *src, void *stream) {
  const char *who = "transferConvert";
  MUGIQ_REQUIRE(dst != nullptr && src != nullptr && dst->V != nullptr && src->V != nullptr, "%s: NULL argument", who);
  for (const MugiqHipTransfer *T : {dst, src}) {
    MUGIQ_REQUIRE(T->precision == 4 || T->precision == 8, "%s: precision %d", who, T->precision);
    MUGIQ_REQUIRE(T->nVec >= 1 && (T->spinBlockSize == 1 || T->spinBlockSize == 2), "%s: nVec = %d, spinBlockSize = %d", who, T->nVec, T->spinBlockSize);
    int64_t vol = 1;
    for (int d = 0; d < 4; d++) {
      MUGIQ_REQUIRE(T->X[d] > 0 && T->geoBlockSize[d] >= 1, "%s: transfer X / geo_block_size[%d]", who, d);
      vol *= T->X[d];
    }
    MUGIQ_REQUIRE(vol % 2 == 0 && T->stride >= vol / 2, "%s: stride = %d is smaller than volumeCB = %lld", who, T->stride, (long long)(vol / 2));
    if (T->spinBlockSize == 2)
      MUGIQ_REQUIRE(T->parity_offset >= (int64_t)12 * T->nVec * T->stride, "%s: parity_offset = %lld is smaller than 12 nVec stride", who,
                    (long long)T->parity_offset);
    else
      MUGIQ_REQUIRE(T->parity_offset > 0 && T->parity_offset % ((int64_t)2 * T->nVec * T->stride) == 0,
                    "%s: a coarse -> coarse transfer needs parity_offset = 2 nc nVec stride exactly, not %lld", who, (long long)T->parity_offset);
  }
  MUGIQ_REQUIRE(dst->nVec == src->nVec && dst->spinBlockSize == src->spinBlockSize, "%s: dst has n_vec %d and spin block %d, src %d and %d", who, dst->nVec,
                dst->spinBlockSize, src->nVec, src->spinBlockSize);
  for (int d = 0; d < 4; d++)
    MUGIQ_REQUIRE(dst->X[d] == src->X[d] && dst->geoBlockSize[d] == src->geoBlockSize[d], "%s: dst has X[%d] = %d and block %d, src %d and %d", who, d,
                  dst->X[d], dst->geoBlockSize[d], src->X[d], src->geoBlockSize[d]);
  const MgLayout Ld = transfer_layout(*dst), Ls = transfer_layout(*src);
  MUGIQ_REQUIRE(Ld.nRows == Ls.nRows, "%s: dst has %d rows per parity, src %d (the colours of the finer side differ)", who, Ld.nRows, Ls.nRows);
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(dst->V), a1 = a0 + (uintptr_t)2 * dst->parity_offset * 2 * dst->precision;
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(src->V), b1 = b0 + (uintptr_t)2 * src->parity_offset * 2 * src->precision;
  MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1), "%s: dst overlaps src", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool wide = debug_wide_index_asked();
  void *dv = const_cast<void *>(dst->V), *sv = const_cast<void *>(src->V);
  MgVecs<double> d8{}, s8{};
  MgVecs<float> d4{}, s4{};
  d8.p[0] = static_cast<Cplx<double> *>(dv), s8.p[0] = static_cast<Cplx<double> *>(sv);
  d4.p[0] = static_cast<Cplx<float> *>(dv), s4.p[0] = static_cast<Cplx<float> *>(sv);
  if (dst->precision == 4 && src->precision == 8) return mg_convert(d4, s8, Ld, Ls, 1, 1u, wide, s);
  if (dst->precision == 8 && src->precision == 4) return mg_convert(d8, s4, Ld, Ls, 1, 1u, wide, s);
  if (dst->precision == 8) return mg_convert(d8, s8, Ld, Ls, 1, 1u, wide, s);
  return mg_convert(d4, s4, Ld, Ls, 1, 1u, wide, s);
}

}  // extern "C"
