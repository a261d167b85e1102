// The Galerkin operator of a coarse -> coarse transfer: M' = R_1 M_c P_1 from the nine matrices K_m(x) of a coarse operator on the lattice
// X1 and the null vectors V of a spin_block_size 1 transfer on it, in the storage of MugiqHipCoarseOperator (so that coarse_apply, the
// eigenpair check and the eigensolver serve it as they stand).  Definition: "the operator of a coarse -> coarse transfer" in
// include/mugiq_hip.h.  Also here: V of such a transfer <-> coarse vectors (the counterparts of csrc/mg_setup.hip's pack kernels).
//
// Numerics (csrc/mg_common.h): products and sums in fp64 whatever the storage, one rounding on the store, no atomics, a summation
// order fixed by the transfer geometry alone -- sites of the aggregate in lexicographic order, per site the terms K_0, +x, -x, ... -t, per
// term the colours of the finer side ascending.
//
// coarse_build2_kernel: a workgroup owns one chirality quadrant (S, S') of one matrix m of one coarsest site.  E(x) is chirality-diagonal,
// so the quadrant needs the quadrant (S, S') of K alone: the four workgroups of a matrix read disjoint quarters, and every K_m(x) leaves
// HBM exactly once per build whatever nc and nv.  Per (x, term): T = K(S, S') V(x'; S') (nc x nv, k = nc) with K and V(x') coming through
// LDS in panels of pk columns / rows, T kept in registers until it is complete and then parked in LDS; then acc += V(x; S)^dag T
// (nv x nv, k = nc) from LDS.  16 x 16 lanes carry 4 x 4 micro-tiles of T and of the output: 8 LDS reads per 16 complex products.
// LDS: (2 nc nv + pk (nc + nv)) complex doubles, 144 KB at nc = nv = 64 with pk = 8.  The vector pipe: a once-per-configuration cost
// (DESIGN.md 4.4f says what the matrix pipe would have bought).
#include "mg_common.h"

#include <algorithm>
#include <vector>

namespace mugiq {
namespace {

constexpr int kC2Threads = 256;  // 16 x 16 lanes
constexpr int kC2Tile = 4;       // ... of 4 x 4 micro-tiles: 64 x 64 elements
constexpr int kC2MaxN = 64;      // nc and nv (kTransferMaxNV: the limit of the operator struct)
constexpr int kC2MinPanel = 8;   // columns of K per panel where LDS is short
constexpr int kC2LdsTarget = 4096;  // complex doubles (64 KB): panels grow up to here, for whole rows of K per read and 2+ workgroups per CU
static_assert(16 * kC2Tile == kC2MaxN && kC2MaxN == kTransferMaxNV, "a quadrant of the largest operator is one micro-tile per lane");
static_assert(sizeof(Cplx<double>) * (size_t)(2 * kC2MaxN * kC2MaxN + kC2MinPanel * 2 * kC2MaxN) <= kTransferMaxLds, "the largest shape fits the LDS of a workgroup");

struct CoarseBuild2Args {
  const void *V;  // [parity][(nc S + c) nv + j][x_cb]
  int64_t Vpo;
  int Vstride, nc, nv;
  TransferGeom g;  // X: the lattice of K, Xc: the coarsest one
  const void *K;   // the finer operator: [site][9][2 nc][2 nc]
  void *out;       // [coarsest site][9][2 nv][2 nv]
  int pk;          // panel width
};

size_t build2_lds_elems(int nc, int nv, int pk) { return (size_t)2 * nc * nv + (size_t)pk * (nc + nv); }
int build2_panel(int nc, int nv) { return std::min(nc, std::max(kC2MinPanel, (kC2LdsTarget - 2 * nc * nv) / (nc + nv))); }

template <typename F> __global__ __launch_bounds__(kC2Threads) void coarse_build2_kernel(CoarseBuild2Args a) {
  extern __shared__ Cplx<double> build2_lds[];
  const int nc = a.nc, nv = a.nv, N0 = 2 * nc, N1 = 2 * nv, pk = a.pk, t = threadIdx.x, tr = t >> 4, tc = t & 15;
  Cplx<double> *Vx = build2_lds, *T = Vx + nc * nv, *Kp = T + nc * nv, *Vp = Kp + nc * pk;  // V(x; S): [nc][nv];  T: [nc][nv];  K: [nc][pk];  V(x'; S'): [pk][nv]
  const int site = blockIdx.x, m = blockIdx.y, S = blockIdx.z >> 1, Sp = blockIdx.z & 1;
  const int cpar = site / a.g.volumeCBc, xc_cb = site - cpar * a.g.volumeCBc;
  int cc[4];
  get_coords(cc, xc_cb, a.g.Xc, cpar);

  // the micro-tiles of this lane: rows tRow of T (colours of the finer side), rows oRow of the output (j), columns col of both (j');
  // lanes past the end shadow the last row / column and do not store
  int tRow[kC2Tile], oRow[kC2Tile], col[kC2Tile];
  Cplx<double> acc[kC2Tile][kC2Tile];
#pragma unroll
  for (int i = 0; i < kC2Tile; i++) {
    tRow[i] = min(kC2Tile * tr + i, nc - 1);
    oRow[i] = min(kC2Tile * tr + i, nv - 1);
    col[i] = min(kC2Tile * tc + i, nv - 1);
#pragma unroll
    for (int k = 0; k < kC2Tile; k++) acc[i][k] = Cplx<double>{0.0, 0.0};
  }

  for (int s = 0; s < a.g.aggVol; s++) {
    int loc[4], x[4], q = s;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      loc[d] = q % a.g.bs[d];
      q /= a.g.bs[d];
      x[d] = cc[d] * a.g.bs[d] + loc[d];
    }
    const int pty = (x[0] + x[1] + x[2] + x[3]) & 1, x_cb = lex_index(x, a.g.X) >> 1;
    bool staged = false;  // V(x; S) is in LDS
    // term 0: K_0(x) against E(x); term 1 + 2 mu: K_{1+2mu}(x) against E(x + mu); term 2 + 2 mu: K_{2+2mu}(x) against E(x - mu).  Xd' takes term
    // 0 and the hops that stay inside the aggregate, Y'+-_mu the one hop that leaves it (every condition is uniform over the workgroup)
    for (int term = (m == 0 ? 0 : m); term <= (m == 0 ? 8 : m); term++) {
      const int mu = (term - 1) >> 1, fwd = term & 1;
      int npty = pty, nidx = x_cb;
      if (term > 0) {
        const bool inside = fwd ? loc[mu] + 1 < a.g.bs[mu] : loc[mu] >= 1;
        if (inside != (m == 0)) continue;
        int dx[4] = {0, 0, 0, 0};
        dx[mu] = fwd ? 1 : -1;
        npty = 1 - pty;
        nidx = link_index_shift(x, dx, a.g.X);
      }
      __syncthreads();  // the products of the previous term have been taken
      if (!staged) {
        for (int i = t; i < nc * nv; i += kC2Threads) Vx[i] = ld_wide<F>(a.V, pty * a.Vpo + (int64_t)(nc * S * nv + i) * a.Vstride + x_cb);
        staged = true;
      }
      // T = K(S, S') V(x'; S'), the colours c' of the neighbour ascending, panel by panel
      const int64_t kbase = (((int64_t)pty * a.g.volumeCB + x_cb) * 9 + term) * N0 * N0 + (int64_t)S * nc * N0 + Sp * nc;
      Cplx<double> tt[kC2Tile][kC2Tile];
#pragma unroll
      for (int i = 0; i < kC2Tile; i++)
#pragma unroll
        for (int k = 0; k < kC2Tile; k++) tt[i][k] = Cplx<double>{0.0, 0.0};
      for (int p0 = 0; p0 < nc; p0 += pk) {
        const int w = min(pk, nc - p0);
        if (p0 > 0) __syncthreads();  // the previous panel is through
        for (int i = t; i < nc * w; i += kC2Threads) {
          const int c0 = i / w, c1 = i - c0 * w;
          Kp[c0 * pk + c1] = ld_wide<F>(a.K, kbase + (int64_t)c0 * N0 + p0 + c1);
        }
        for (int i = t; i < w * nv; i += kC2Threads) Vp[i] = ld_wide<F>(a.V, npty * a.Vpo + (int64_t)((nc * Sp + p0) * nv + i) * a.Vstride + nidx);
        __syncthreads();
#pragma unroll 2
        for (int c1 = 0; c1 < w; c1++) {
          Cplx<double> kk[kC2Tile], vv[kC2Tile];
#pragma unroll
          for (int i = 0; i < kC2Tile; i++) {
            kk[i] = Kp[tRow[i] * pk + c1];
            vv[i] = Vp[c1 * nv + col[i]];
          }
#pragma unroll
          for (int i = 0; i < kC2Tile; i++)
#pragma unroll
            for (int k = 0; k < kC2Tile; k++) cmadd(tt[i][k], kk[i], vv[k]);
        }
      }
#pragma unroll
      for (int i = 0; i < kC2Tile; i++)
#pragma unroll
        for (int k = 0; k < kC2Tile; k++)
          if (kC2Tile * tr + i < nc && kC2Tile * tc + k < nv) T[(kC2Tile * tr + i) * nv + kC2Tile * tc + k] = tt[i][k];
      __syncthreads();
      // acc += V(x; S)^dag T
#pragma unroll 2
      for (int c0 = 0; c0 < nc; c0++) {
        Cplx<double> xx[kC2Tile], yy[kC2Tile];
#pragma unroll
        for (int i = 0; i < kC2Tile; i++) {
          xx[i] = Vx[c0 * nv + oRow[i]];
          yy[i] = T[c0 * nv + col[i]];
        }
#pragma unroll
        for (int i = 0; i < kC2Tile; i++)
#pragma unroll
          for (int k = 0; k < kC2Tile; k++) cmadd_conj(acc[i][k], xx[i], yy[k]);
      }
    }
  }
  const int64_t obase = ((int64_t)site * 9 + m) * N1 * N1 + (int64_t)S * nv * N1 + Sp * nv;
#pragma unroll
  for (int i = 0; i < kC2Tile; i++)
#pragma unroll
    for (int k = 0; k < kC2Tile; k++)
      if (kC2Tile * tr + i < nv && kC2Tile * tc + k < nv) st_round<F>(a.out, obase + (int64_t)(kC2Tile * tr + i) * N1 + kC2Tile * tc + k, acc[i][k]);
}

template <typename F> int launch_build2(const MugiqHipCoarseOperator *op, const MugiqHipTransfer *T, const MugiqHipCoarseOperator *finer, hipStream_t stream) {
  CoarseBuild2Args a;
  a.V = T->V;
  a.Vpo = T->parity_offset;
  a.Vstride = T->stride;
  a.nc = finer->nVec;
  a.nv = T->nVec;
  a.g = transfer_geom(*T);
  a.K = finer->data;
  a.out = op->data;
  a.pk = build2_panel(a.nc, a.nv);
  const size_t lds = sizeof(Cplx<double>) * build2_lds_elems(a.nc, a.nv, a.pk);
  if (lds > kTransferMaxLds)  // (not reachable for nc, nv <= 64: the static_assert above)
    return set_error(MUGIQ_HIP_ERROR_UNSUPPORTED, "computeCoarseOperatorCoarse: %zu bytes of LDS for nc = %d, n_vec = %d", lds, a.nc, a.nv);
  return launch_with_lds(coarse_build2_kernel<F>, dim3((unsigned)(2 * a.g.volumeCBc), 9, 4), kC2Threads, lds, stream, a);
}

// ---- V of a coarse -> coarse transfer <-> coarse vectors.  One lane per (parity, plane k = nc s + c, x_cb) ---------------------------
struct Pack2Args {
  void *V;
  int64_t po;
  int stride, nVec, volumeCB;
  const void *const *vecs;  // device table of the vectors' bodies (pack)
  void *vec;                // the one vector (unpack)
  int j, fStride;
  int64_t fPo;
};
template <typename FV, typename FS> __global__ __launch_bounds__(256) void pack_coarse_vectors_kernel(Pack2Args A) {
  const int x = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, parity = blockIdx.z;
  if (x >= A.volumeCB) return;
  const int64_t src = parity * A.fPo + (int64_t)k * A.fStride + x, dst = parity * A.po + (int64_t)k * A.nVec * A.stride + x;
  for (int j = 0; j < A.nVec; j++) st_round<FV>(A.V, dst + (int64_t)j * A.stride, ld_wide<FS>(as_constant(A.vecs)[j], src));
}
template <typename FV, typename FS> __global__ __launch_bounds__(256) void unpack_coarse_vector_kernel(Pack2Args A) {
  const int x = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, parity = blockIdx.z;
  if (x >= A.volumeCB) return;
  st_round<FS>(A.vec, parity * A.fPo + (int64_t)k * A.fStride + x, ld_wide<FV>(A.V, parity * A.po + ((int64_t)k * A.nVec + A.j) * A.stride + x));
}

// the transfer of a coarse -> coarse level on its own: geometry, and the colours nc of its finer side from parity_offset = 2 nc n_vec stride
int check_coarse_level(const MugiqHipTransfer *T, const char *who, int *ncOut) {
  MUGIQ_REQUIRE(T->V != nullptr, "%s: transfer / null vectors are NULL", who);
  MUGIQ_REQUIRE(T->spinBlockSize == 1, "%s: spin_block_size = %d: a coarse -> coarse transfer (1) is needed", who, T->spinBlockSize);
  MUGIQ_REQUIRE(T->precision == 4 || T->precision == 8, "%s: transfer precision %d", who, T->precision);
  MUGIQ_REQUIRE(T->nVec >= 1 && T->nVec <= kC2MaxN, "%s: n_vec = %d must be in [1, %d]", who, T->nVec, kC2MaxN);
  long long vol = 1;
  for (int d = 0; d < 4; d++) {
    MUGIQ_REQUIRE(T->X[d] > 0 && (T->X[d] & 1) == 0, "%s: finer lattice X[%d] = %d must be positive and even", who, d, T->X[d]);
    MUGIQ_REQUIRE(T->geoBlockSize[d] >= 1 && T->X[d] % T->geoBlockSize[d] == 0, "%s: geo_block_size[%d] = %d does not divide X = %d", who, d,
                  T->geoBlockSize[d], T->X[d]);
    MUGIQ_REQUIRE(((T->X[d] / T->geoBlockSize[d]) & 1) == 0, "%s: coarsest extent %d in dim %d must be even", who, T->X[d] / T->geoBlockSize[d], d);
    vol *= T->X[d];
  }
  MUGIQ_REQUIRE(vol / 2 < (1LL << 30), "%s: volume overflows int", who);
  MUGIQ_REQUIRE(T->stride >= vol / 2, "%s: V stride %d is smaller than volumeCB = %lld", who, T->stride, vol / 2);
  const int64_t unit = (int64_t)2 * T->nVec * T->stride;
  MUGIQ_REQUIRE(T->parity_offset >= unit && T->parity_offset % unit == 0 && T->parity_offset / unit <= kC2MaxN,
                "%s: a coarse -> coarse V must have parity_offset = 2 nColor n_vec stride with nColor in [1, %d] (it is %lld, 2 n_vec stride = %lld)", who,
                kC2MaxN, (long long)T->parity_offset, (long long)unit);
  *ncOut = (int)(T->parity_offset / unit);
  return MUGIQ_HIP_SUCCESS;
}

// n coarse vectors on the finer side of T (nc colours), of one layout
int check_pack2(const MugiqHipTransfer *T, const MugiqHipCoarseField *v, int n, const char *who, int *ncOut) {
  MUGIQ_REQUIRE(T != nullptr && v != nullptr, "%s: NULL argument", who);
  if (int st = check_coarse_level(T, who, ncOut)) return st;
  const int nc = *ncOut;
  long long vol = 1;
  for (int d = 0; d < 4; d++) vol *= T->X[d];
  for (int i = 0; i < n; i++) {
    const MugiqHipCoarseField &w = v[i];
    MUGIQ_REQUIRE(w.data != nullptr, "%s: vector %d is NULL", who, i);
    MUGIQ_REQUIRE(w.precision == 4 || w.precision == 8, "%s: vector %d has precision %d", who, i, w.precision);
    MUGIQ_REQUIRE(w.nSpin == 2 && w.nColor == nc, "%s: vector %d has nSpin %d, nColor %d; the transfer's finer side has nSpin 2, nColor %d", who, i, w.nSpin,
                  w.nColor, nc);
    for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(w.X[d] == T->X[d], "%s: vector %d: X[%d] = %d, the transfer's is %d", who, i, d, w.X[d], T->X[d]);
    MUGIQ_REQUIRE(w.volumeCB == (int)(vol / 2) && w.stride >= w.volumeCB && w.parity_offset >= (int64_t)2 * w.nColor * w.stride,
                  "%s: vector %d: volumeCB / stride / parity_offset", who, i);
    MUGIQ_REQUIRE(w.precision == v[0].precision && w.stride == v[0].stride && w.parity_offset == v[0].parity_offset,
                  "%s: vector %d differs in precision or layout from vector 0", who, i);
  }
  return MUGIQ_HIP_SUCCESS;
}

Pack2Args pack2_args(const MugiqHipTransfer *T, const MugiqHipCoarseField &v) {
  Pack2Args A{};
  A.V = const_cast<void *>(T->V);
  A.po = T->parity_offset;
  A.stride = T->stride, A.nVec = T->nVec, A.volumeCB = v.volumeCB;
  A.fStride = v.stride, A.fPo = v.parity_offset;
  return A;
}
inline dim3 pack2_grid(const Pack2Args &A, int nc) { return dim3((unsigned)((A.volumeCB + 255) / 256), (unsigned)(2 * nc), 2); }

}  // namespace
}  // namespace mugiq

using namespace mugiq;

extern "C" {

int mugiq_hip_compute_coarse_operator_coarse(MugiqHipCoarseOperator *op, const MugiqHipTransfer *transfer, const MugiqHipCoarseOperator *finerOp,
                                             const MugiqHipComm *comm, void *stream) {
  const char *who = "computeCoarseOperatorCoarse";
  // ---- validation, before any device work
  MUGIQ_REQUIRE(op != nullptr && transfer != nullptr && finerOp != nullptr, "%s: NULL argument", who);
  int st, nc = 0;
  if ((st = check_single_domain(comm, who))) return st;
  if ((st = check_coarse_level(transfer, who, &nc))) return st;
  if ((st = validate_coarse_operator(finerOp, who))) return st;
  if ((st = validate_coarse_operator(op, who))) return st;
  for (int d = 0; d < 4; d++)
    MUGIQ_REQUIRE(transfer->X[d] == finerOp->X[d], "%s: transfer X[%d] = %d, the finer operator's lattice has %d", who, d, transfer->X[d], finerOp->X[d]);
  MUGIQ_REQUIRE(nc == finerOp->nVec, "%s: parity_offset = %lld gives the finer side %d colours (2 nColor n_vec stride), the finer operator has n_vec %d", who,
                (long long)transfer->parity_offset, nc, finerOp->nVec);
  MUGIQ_REQUIRE(op->precision == transfer->precision, "%s: the coarse operator has precision %d, the transfer %d", who, op->precision, transfer->precision);
  MUGIQ_REQUIRE(finerOp->precision == transfer->precision, "%s: the finer operator has precision %d, the transfer %d", who, finerOp->precision,
                transfer->precision);
  MUGIQ_REQUIRE(op->nVec == transfer->nVec, "%s: the coarse operator has n_vec %d, the transfer %d", who, op->nVec, transfer->nVec);
  for (int d = 0; d < 4; d++)
    MUGIQ_REQUIRE(op->X[d] == transfer->X[d] / transfer->geoBlockSize[d], "%s: coarse operator X[%d] = %d, the transfer's coarse lattice has %d", who, d,
                  op->X[d], transfer->X[d] / transfer->geoBlockSize[d]);
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(op->data), a1 = a0 + mugiq_hip_coarse_operator_bytes(op->X, op->nVec, op->precision);
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(finerOp->data), b1 = b0 + mugiq_hip_coarse_operator_bytes(finerOp->X, finerOp->nVec, finerOp->precision);
  MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1), "%s: the coarse operator's data overlaps the finer operator's", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  st = transfer->precision == 8 ? launch_build2<double>(op, transfer, finerOp, s) : launch_build2<float>(op, transfer, finerOp, s);
  if (st) return st;
  op->kappa = finerOp->kappa;
  op->hasClover = finerOp->hasClover;
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_transfer_set_coarse_vectors(const MugiqHipTransfer *transfer, const MugiqHipCoarseField *vecs_h, int nVec, void *stream) {
  const char *who = "transferSetCoarseVectors";
  MUGIQ_REQUIRE(transfer != nullptr && vecs_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nVec == transfer->nVec, "%s: %d vectors for a transfer of n_vec = %d", who, nVec, transfer->nVec);
  int nc = 0;
  if (int st = check_pack2(transfer, vecs_h, nVec, who, &nc)) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<const void *> host(nVec);
  for (int j = 0; j < nVec; j++) host[j] = vecs_h[j].data;
  void *table = nullptr;
  if (int st = upload_table(&table, host.data(), sizeof(void *) * host.size(), s)) return st;
  Pack2Args A = pack2_args(transfer, vecs_h[0]);
  A.vecs = static_cast<const void *const *>(table);
  with_storage(transfer->precision, vecs_h[0].precision, [&](auto fv, auto fs) {
    hipLaunchKernelGGL((pack_coarse_vectors_kernel<decltype(fv), decltype(fs)>), pack2_grid(A, nc), dim3(256), 0, s, A);
  });
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

int mugiq_hip_transfer_get_coarse_vector(const MugiqHipCoarseField *vec, const MugiqHipTransfer *transfer, int j, void *stream) {
  const char *who = "transferGetCoarseVector";
  int nc = 0;
  if (int st = check_pack2(transfer, vec, 1, who, &nc)) return st;
  MUGIQ_REQUIRE(j >= 0 && j < transfer->nVec, "%s: j = %d is not in [0, n_vec = %d)", who, j, transfer->nVec);
  hipStream_t s = static_cast<hipStream_t>(stream);
  Pack2Args A = pack2_args(transfer, *vec);
  A.vec = vec->data, A.j = j;
  with_storage(transfer->precision, vec->precision, [&](auto fv, auto fs) {
    hipLaunchKernelGGL((unpack_coarse_vector_kernel<decltype(fv), decltype(fs)>), pack2_grid(A, nc), dim3(256), 0, s, A);
  });
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

}  // extern "C"
