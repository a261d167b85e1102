// Internal helpers shared by the HIP translation units of libmugiq_hip.so (gfx950 only).  What only the multigrid translation units
// share (storage access, the aggregate and Galerkin term walks, launch helpers) is in csrc/mg_common.h, on top of this file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "fused_form.h"
#include "mugiq_hip.h"
#include "transfer_form.h"

namespace mugiq {

// ---- error plumbing ------------------------------------------------------------------------------
int set_error(int status, const char *fmt, ...);
#define MUGIQ_CHECK_HIP(call)                                                                     \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return ::mugiq::set_error(MUGIQ_HIP_ERROR_HIP, "%s:%d: %s failed: %s", __FILE__, __LINE__,  \
                                #call, hipGetErrorString(e_));                                    \
  } while (0)
#define MUGIQ_REQUIRE(cond, ...)                                                                  \
  do {                                                                                            \
    if (!(cond)) return ::mugiq::set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, __VA_ARGS__);        \
  } while (0)

// Per-(device, stream) scratch (host_api.cpp).  Small tables (pointer lists, 1/sigma, momenta) go through
// upload_table: a pinned staging copy, then an H2D copy ordered on `stream`, so the caller's memory may be released
// on return.  Successive calls on one stream reuse the same buffer -- safe because the stream orders the next upload
// behind the previous kernel; calls on different streams (or threads, or Loop objects) never share one.
// stream_scratch returns the table buffer itself (at least `bytes` large; the next upload_table of at most that size
// on the same stream lands at the same address); stream_workspace is a second, independent buffer of the same arena.
// Who may hold which: a reservation is good until the next request for the same buffer on the stream (a larger one moves it).  So a
// solver or a check reserves once, before its first launch, and calls internal entries only: the stencil, the restrictions and the
// prolongations below (stencil_apply, restrict_*, prolong_*) take their work memory from the caller and reserve nothing; they upload
// tables, which live for the launches that follow.  coarse_apply alone keeps the intermediate of a normal form in stream_workspace: its
// callers keep their own vectors in the operator workspace.
int stream_scratch(void **ptr, size_t bytes, hipStream_t stream);
int stream_workspace(void **ptr, size_t bytes, hipStream_t stream);
int upload_table(void **dev, const void *host, size_t bytes, hipStream_t stream);
// ... the table every fused entry reads: the bodies of ev[0 .. nVec) (then, two-sided, of evL), and behind them 1/sigma as float or
// double (tablePrecision 4 | 8).  sigmaPrecision 4: sigma rounded to float before it is inverted (the vector kernels over fp32 storage)
int upload_vector_table(const void *const **L, const void **invSigma, const MugiqHipSpinorField *ev, const MugiqHipSpinorField *evL,
                        const double *sigma, int nVec, int sigmaPrecision, int tablePrecision, hipStream_t stream);
// a third buffer of the arena, for the operators and solvers (csrc/wilson.hip, csrc/mg_solve.hip, the explicit coarse check of
// csrc/restrict.hip): intermediate and solver vectors that must survive the calls of the deflation and halo code and of coarse_apply in
// between, which use stream_workspace themselves.  Held by one public call at a time, which calls no other holder while it holds it
int stream_operator_workspace(void **ptr, size_t bytes, hipStream_t stream);
int release_stream_scratch(hipStream_t stream);
size_t eo_dft_x_lds_bytes(int precision, const int localL[4], int nPx, int *redOffsetElems);  // momproj.hip
int eo_dft_x_time_chunk(int precision, const int localL[4], int nPx);                            // momproj.hip: 0 = the fused x step does not apply
int fill_identity_links(const MugiqHipSpinorField *f, hipStream_t stream);  // displace.hip
// MUGIQ_HIP_DEBUG_POISON_LDS=1 (test aid): every compute entry point of the C ABI first overwrites the LDS of all CUs with NaN bit
// patterns (mugiq_hip_debug_poison_lds), so that a kernel reading a cell it never wrote shows it in its result.  A solver or a check
// does the same in front of every stencil, restriction and prolongation of its own (the internal entries below do not)
int debug_poison_lds_if_asked(hipStream_t stream);
// MUGIQ_HIP_DEBUG_WIDE_INDEX=1 (test aid): the Krylov kernels of csrc/mg_solve.hip run in their int64_t instantiation whatever the size
// of the field (otherwise only from 2^31 complex elements per vector on, 32 GiB, which no test reaches).  Read by every call of
// mugiq_hip_mg_solve / mugiq_hip_mg_precondition, of their mixed-precision twins and of the two conversions; the order of every sum depends on the shape alone, so the results are the same bits.
bool debug_wide_index_asked();
// csrc/fused_mfma.hip.  The axial gauge of a (direction, sign) is rebuilt by every call of the matrix-pipe tile (one pass over
// W_1, 0.2 ms) -- unless the caller, who calls the same entry several times (the driver: interior tiles, then the boundary tiles
// block by block), has built it once and hands it over (FusedEntryPlan::axialGauge; FusedForm::gaugeBytes large).
int build_axial_gauge(void *G_d, const MugiqHipSpinorField &ev, const void *const *E_d, int kmax, int dir, int sign, hipStream_t stream);
// ... straight from the gauge field (no path-link fields needed at all): where axial_gauge_from_links_possible (csrc/fused_form.h)
int build_axial_gauge_from_links(void *G_d, const MugiqHipSpinorField &ev, const MugiqHipGaugeField &U, int kmax, int dir, int sign, hipStream_t stream);
// The tile is exact only where g^dag g = 1.  axial_gauge_tolerance: the largest deviation max |g^dag g - 1| it is taken with
// (per storage precision).  axial_line_deviation: the driver's pre-pass, D[mu] over the lines of the local gauge field out to reach[mu]
// positions past both ends (reach 0: D = 0, not looked at); blocks the host once.  build_axial_gauge_checked: the free fused call's
// gauge from its links, built into the stream's workspace, with its deviation; blocks the host once.
double axial_gauge_tolerance(int precision);
int axial_line_deviation(double D[4], const MugiqHipGaugeField &U, const int reach[4], const int partitioned[4], hipStream_t stream);
int build_axial_gauge_checked(void **G_out, double *deviation, const MugiqHipSpinorField &ev, const void *const *E_d, int kmax, int dir, int sign,
                              hipStream_t stream);

// Face layers packed by a mu = x entry on its way through the eigenvectors (csrc/fused_mfma.hip, row tile): the driver hands the
// targets of the halos it is about to post to the entry that runs first, instead of launching mugiq_hip_pack_face_layers beside it
// (the pack kernels and a tile kernel that fills every CU's registers and LDS take turns, they do not overlap).
// Layout of out_d: [nVec][layers][parity][12][faceCB], what mugiq_hip_pack_face_layers writes.
struct EntryPackTarget {
  void *out_d;
  int dim;     // 2 | 3
  int high;    // 0: layers x[dim] = j | 1: x[dim] = X - 1 - j
  int layers;
  int fromVec;  // eigenvectors fromVec .. nVec - 1 (the ones before went out packed by mugiq_hip_pack_face_layers)
};
// What the driver tells the fused calls of one entry that the public C call cannot express (NULL plan: a free call)
struct FusedEntryPlan {
  int tile = -1;                     // 1 the tile may be taken (the driver's pre-pass passed), 0 it may not (the vector tiles take the entry),
                                     // -1 no decision (a free call: fused_entry checks the gauge of W_1 .. W_kmax itself)
  const void *axialGauge = nullptr;  // the gauge the caller built for (dir, sign, kmax of the call): the tile must take the call, and the
                                     // link fields are not read (pathLinkFields_h may be NULL)
  const EntryPackTarget *pack = nullptr;  // face layers for the first launch of the row tile to write (at most FusedForm::packCapacity)
  int nPack = 0;
  bool *packed = nullptr;  // with pack: set once a launch has taken the targets (later calls of the entry leave them alone)
  const FusedForm *form = nullptr;  // the kernel form the driver's plan chose for the entry (NULL: fused_entry selects)
};
// The matrix-pipe tile (fourth generation, any storage type, ascending lengths up to 8) of an entry whose form is one.  evL != NULL: the
// two-sided tile (no 12-position column tile, 8-wave row tile only).  G_d: the axial gauge of the call (NULL: built here from E_d);
// pack / nPack / packed: as in FusedEntryPlan
int mfma_tile_entry(const FusedForm &form, void *loop_d, const MugiqHipSpinorField *ev, const double *sigma, int nVec, const void *const *E_d,
                    const int *kvals, int nK, int sign, const void *ghost_d, int layers, int region,
                    hipStream_t stream, void *ultra_d, int *carried, const MugiqHipSpinorField *evL, const void *G_d,
                    const EntryPackTarget *pack, int nPack, bool *packed);
// csrc/fused.hip: what mugiq_hip_displaced_loop_contraction_fused_carry (eVecL_h = NULL) and ..._fused_two_sided do, and which kernel
// did it (*kernel = MUGIQ_HIP_ENTRY_KERNEL_*; may be NULL).  The two-sided form runs on the matrix-pipe tile only: where that does not
// apply it fails with MUGIQ_HIP_ERROR_UNSUPPORTED (the driver's plan asks select_fused_form first and takes the step-by-step sequence)
int fused_contraction(void *loopData_d, int loopPrecision, const MugiqHipSpinorField *eVecL_h, const MugiqHipSpinorField *eVecR_h,
                      const double *sigma_h, int nVec, const void *const *pathLinkFields_h, const int *kValues_h, int nK, int dispDir,
                      int dispSign, const int commDim[4], const void *ghostLayers_d, int layers, int region, void *ultraLocalSlot_d,
                      int *carried, void *stream, int *kernel, const FusedEntryPlan *plan);
// csrc/deflate.hip: mugiq_hip_deflate_low_modes with the caller's name in the messages (mugiq_hip_loop_deflate passes the loop's set)
int deflate_low_modes(const MugiqHipSpinorField *dst, const MugiqHipSpinorField *src, int nVec, const MugiqHipSpinorField *ev,
                      const double *sigma, int nEv, int gamma5, double *overlaps_h, const MugiqHipComm *comm, hipStream_t stream,
                      const char *who);
// csrc/prolong.hip: a finest-level transfer against the first coarse field of a call; one coarse -> coarse level against the nVec
// fields of its finer and coarser side (both shared with the restriction, csrc/restrict.hip)
int validate_transfer(const MugiqHipTransfer *T, const MugiqHipCoarseField *c0, const char *who);
int validate_coarse_transfer(const MugiqHipTransfer *T, const MugiqHipCoarseField *finer_h, const MugiqHipCoarseField *coarser_h, int nVec,
                             const char *who);
// The transfers behind the validation of their extern "C" entries (mugiq_hip_prolongate_batched, ..._coarse_batched, csrc/prolong.hip;
// mugiq_hip_restrict_batched, ..._coarse_batched, csrc/restrict.hip), for callers that validated their hierarchy up front.
// prolong_batched runs the form select_prolong_form gives for `sw`; packed_ws: that form's workspaceBytes, the caller's
int prolong_batched(const MugiqHipSpinorField *fine, const MugiqHipCoarseField *coarse, int nVec, const MugiqHipTransfer *T, const TransferSwitches &sw,
                    void *packed_ws, hipStream_t stream);
int prolong_coarse_batched(const MugiqHipCoarseField *out, const MugiqHipCoarseField *in, int nVec, const MugiqHipTransfer *T, hipStream_t stream);
int restrict_batched(const MugiqHipCoarseField *coarse, const MugiqHipSpinorField *fine, int nVec, const MugiqHipTransfer *T, int gamma5, hipStream_t stream);
int restrict_coarse_batched(const MugiqHipCoarseField *coarser, const MugiqHipCoarseField *finer, int nVec, const MugiqHipTransfer *T, hipStream_t stream);
// csrc/coarse_op.hip: a finest-level transfer (validate_transfer against the coarse side it lays out itself) and the coarse operator built
// from it: one precision, one n_vec, the operator on the transfer's coarse lattice.  T->V and op are the caller's to check first
int validate_transfer_operator(const MugiqHipTransfer *T, const MugiqHipCoarseOperator *op, const char *who);
// csrc/restrict.hip: mugiq_hip_deflate_low_modes_coarse with the caller's name in the messages (mugiq_hip_loop_deflate_coarse passes the
// loop's coarse set and transfers)
int deflate_low_modes_coarse(const MugiqHipSpinorField *dst, const MugiqHipSpinorField *src, int nVec, const MugiqHipCoarseField *ev,
                             const double *sigma, int nEv, const MugiqHipTransfer *transfers, int nLevels, int gamma5, double *overlaps_h,
                             const MugiqHipComm *comm, hipStream_t stream, const char *who);
// csrc/coarse_op.hip: the explicit coarse operator.  check_single_domain: MUGIQ_HIP_ERROR_UNSUPPORTED for a comm with more than one rank
// or a partitioned axis; validate_coarse_vectors: n fields the operator can act on, of one stride and parity offset; coarse_apply:
// mugiq_hip_coarse_apply behind its validation (the eigenpair check of csrc/restrict.hip calls it block by block)
int check_single_domain(const MugiqHipComm *comm, const char *who);
int validate_coarse_operator(const MugiqHipCoarseOperator *op, const char *who);
int validate_coarse_vectors(const MugiqHipCoarseField *f, int n, const MugiqHipCoarseOperator *op, const char *who, const char *name);
int coarse_apply(const MugiqHipCoarseField *dst, const MugiqHipCoarseField *src, int nVec, const MugiqHipCoarseOperator *op, int opType, double scale,
                 hipStream_t stream);
// ... on a process grid.  check_coarse_grid: comm -> part[4] (check_comm), a valid operator, and the halo of that operator built for every
// partitioned axis (NULL only where nothing is partitioned), before any device work; coarse_apply_grid: mugiq_hip_coarse_apply_grid behind
// its validation.  With part all 0 it is coarse_apply
int check_coarse_grid(const MugiqHipComm *comm, const MugiqHipCoarseOperator *op, const MugiqHipCoarseHalo *halo, int part[4], bool needSums,
                      const char *who);
// coarse_grid_layout: where coarse_apply_grid keeps its work memory, as byte offsets from the start of stream_workspace (send: the low
// [0] and the high [1] face of a partitioned axis, in the layout of face_pack_kernel; cap: bytes of one face buffer, 0 where the axis is
// not partitioned).  A caller that reserves `bytes` or more once (a reservation of the largest size stays where it is) knows the
// addresses of every later call with the same operator, axes, form and min(nVec, 8): the coarse eigensolver writes the send faces of the
// next application from its recurrence kernel and passes firstPacked, which makes the first launch exchange them as they are.
// counts (may be NULL): the exchanges issued and the launches of face_pack_kernel made are added
struct CoarseGridLayout {
  size_t bytes, intermediate;
  size_t send[4][2], recv[4][2], cap[4];
  int faceCB[4];
};
struct CoarseGridCounts {
  int exchanges = 0, packLaunches = 0;
};
void coarse_grid_layout(CoarseGridLayout *L, const MugiqHipCoarseOperator *op, const int part[4], int opType, int nVec);
int coarse_apply_grid(const MugiqHipCoarseField *dst, const MugiqHipCoarseField *src, int nVec, const MugiqHipCoarseOperator *op,
                      const MugiqHipCoarseHalo *halo, const int part[4], int opType, double scale, const MugiqHipComm *comm, hipStream_t stream,
                      bool firstPacked = false, CoarseGridCounts *counts = nullptr);
// csrc/wilson.hip: the gauge field of an operator call against the local dims X and the partitioned axes; comm -> part[4]
int check_gauge(const MugiqHipGaugeField *U, const int X[4], const int part[4], const char *who);
int check_comm(const MugiqHipComm *comm, int part[4], bool needSums, const char *who);
// ... and the stencil behind those checks.  OpContext: the operator of a call and where its halo exchange packs: stencil_send_bytes for
// the most fields one stencil_apply of the call takes, laid out like `like` in precision prec (0 on a single domain: send may be NULL).
// stencil_apply: dst_i = scale [g5] M^(dag) src_i for n fields of one layout; the ghost zones of src are exchanged first
struct OpContext {
  const MugiqHipGaugeField *U;
  const MugiqHipComm *comm;
  int part[4];
  double kappa;
  hipStream_t stream;
  unsigned char *send;
  const char *who;
  const MugiqHipCloverField *clover = nullptr;  // NULL: the unimproved operator
};
size_t stencil_send_bytes(const MugiqHipSpinorField &like, int prec, const int part[4], int n);
// ... and the bytes one ghost zone of axis d takes where a caller carves the zones of a field one behind the other ([d][low, high], the
// partitioned axes only): together the stencil_send_bytes of one field
size_t stencil_zone_bytes(const MugiqHipSpinorField &like, int prec, int d);
int stencil_apply(const OpContext &c, const MugiqHipSpinorField *dst, const MugiqHipSpinorField *src, int n, int dagger, int gamma5, double scale);
// csrc/clover.hip: descriptor bounds; X != NULL: and the geometry of the fields it is applied to
int validate_clover(const MugiqHipCloverField *C, const int X[4], int volumeCB, const char *who);
}  // namespace mugiq
#include <vector>
namespace mugiq {
bool momenta_negation_table(const int *mom, int Nmom, std::vector<int> &neg);  // reflect_mom.cpp
// csrc/deflate.hip: c <- the sum of c over all ranks, in the fixed order of the momentum projection (reduce over space, gather over
// time, rank-ordered sum on the root, bcast): identical bits on every rank
int sum_over_ranks(const MugiqHipComm *comm, std::vector<double> &c);

// ---- address spaces ---------------------------------------------------------------------------------------------
// Pointers fetched from a device-side table (eigenvector bodies) have no known address space, so hipcc emits
// flat_load: those count on vmcnt AND lgkmcnt and return out of order, which forces one `s_waitcnt vmcnt(0)
// lgkmcnt(0)` in front of the first use -- no load can overlap arithmetic inside a wave.  Casting to the global
// address space turns them into global_load (ordered, counted waits).
#define MUGIQ_GLOBAL __attribute__((address_space(1)))
template <typename T> __device__ inline const MUGIQ_GLOBAL T *as_global(const T *p) { return (const MUGIQ_GLOBAL T *)p; }
template <typename T> __device__ inline MUGIQ_GLOBAL T *as_global(T *p) { return (MUGIQ_GLOBAL T *)p; }
// Tables the host uploads before the launch and the kernel never writes (pointer / 1/sigma tables): the constant
// address space lets hipcc fetch a wave-uniform entry with s_load (lgkmcnt) instead of a vector load, which would
// share the in-order vmcnt queue with the prefetched eigenvector loads and drain it at every use.
#define MUGIQ_CONSTANT __attribute__((address_space(4)))
template <typename T> __device__ inline const MUGIQ_CONSTANT T *as_constant(const T *p) { return (const MUGIQ_CONSTANT T *)p; }

// ---- complex arithmetic in registers -------------------------------------------------------------
template <typename F> struct alignas(2 * sizeof(F)) Cplx {
  F re, im;
};
// a += conj(x) * y
template <typename F> __device__ inline void cmadd_conj(Cplx<F> &a, const Cplx<F> &x, const Cplx<F> &y) {
  a.re = fma(x.re, y.re, a.re);
  a.re = fma(x.im, y.im, a.re);
  a.im = fma(x.re, y.im, a.im);
  a.im = fma(-x.im, y.re, a.im);
}
// a += x * y
template <typename F> __device__ inline void cmadd(Cplx<F> &a, const Cplx<F> &x, const Cplx<F> &y) {
  a.re = fma(x.re, y.re, a.re);
  a.re = fma(-x.im, y.im, a.re);
  a.im = fma(x.re, y.im, a.im);
  a.im = fma(x.im, y.re, a.im);
}

// ---- DeGrand-Rossi gamma tables, include/gamma.h:32-71 of the reference ----------------------------
// G(n)_{ij} = value[n][i] * delta(j, column[n][i]); value in {+1,-1,+i,-i} encoded as a power of i:
// 0 -> +1, 1 -> +i, 2 -> -1, 3 -> -i.
constexpr int kGammaPhase[16][4] = {
    {0, 0, 0, 0}, {1, 1, 3, 3}, {2, 0, 0, 2}, {3, 1, 3, 1}, {1, 3, 3, 1}, {2, 0, 2, 0}, {3, 3, 3, 3}, {0, 0, 2, 2},
    {0, 0, 0, 0}, {1, 1, 3, 3}, {2, 0, 0, 2}, {3, 1, 3, 1}, {1, 3, 3, 1}, {2, 0, 2, 0}, {3, 3, 3, 3}, {0, 0, 2, 2}};
constexpr int kGammaColumn[16][4] = {
    {0, 1, 2, 3}, {3, 2, 1, 0}, {3, 2, 1, 0}, {0, 1, 2, 3}, {2, 3, 0, 1}, {1, 0, 3, 2}, {1, 0, 3, 2}, {2, 3, 0, 1},
    {2, 3, 0, 1}, {1, 0, 3, 2}, {1, 0, 3, 2}, {2, 3, 0, 1}, {0, 1, 2, 3}, {3, 2, 1, 0}, {3, 2, 1, 0}, {0, 1, 2, 3}};
// G -> g5*G map, include/gamma.h:99-109: index[ig] = 15 - ig, sign = -1 for ig in {3,6,9,11,12,14}
constexpr int kGammaMapSign[16] = {1, 1, 1, -1, 1, 1, -1, 1, 1, -1, 1, -1, -1, 1, -1, 1};

// t += i^phase * z
template <typename F> __device__ inline void add_phase(Cplx<F> &t, int phase, const Cplx<F> &z) {
  switch (phase) {
  case 0: t.re += z.re; t.im += z.im; break;
  case 1: t.re -= z.im; t.im += z.re; break;
  case 2: t.re -= z.re; t.im -= z.im; break;
  default: t.re += z.im; t.im -= z.re; break;
  }
}

// ---- per-site contraction arithmetic shared by the contraction, fused and prolong-contract kernels -----------
// acc (full 4x4) += conj(l[be,c]) * (s * r[al,c])
template <typename F> __device__ inline void accumulate_full(Cplx<F> acc[16], const Cplx<F> l[12], const Cplx<F> r[12], F s) {
  Cplx<F> sr[12];
#pragma unroll
  for (int k = 0; k < 12; k++) sr[k] = Cplx<F>{s * r[k].re, s * r[k].im};
#pragma unroll
  for (int be = 0; be < 4; be++)
#pragma unroll
    for (int al = 0; al < 4; al++)
#pragma unroll
      for (int c = 0; c < 3; c++) cmadd_conj(acc[be * 4 + al], l[be * 3 + c], sr[al * 3 + c]);
}

// Hermitian case (l == r): diagonal kept in diag[4] (real), strict upper triangle in up[6]
// pair order (be,al): (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
template <typename F> __device__ inline void accumulate_herm(F diag[4], Cplx<F> up[6], const Cplx<F> v[12], F s) {
  Cplx<F> sv[12];
#pragma unroll
  for (int k = 0; k < 12; k++) sv[k] = Cplx<F>{s * v[k].re, s * v[k].im};
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      diag[a] = fma(v[a * 3 + c].re, sv[a * 3 + c].re, diag[a]);
      diag[a] = fma(v[a * 3 + c].im, sv[a * 3 + c].im, diag[a]);
    }
  int p = 0;
#pragma unroll
  for (int be = 0; be < 4; be++)
#pragma unroll
    for (int al = be + 1; al < 4; al++) {
#pragma unroll
      for (int c = 0; c < 3; c++) cmadd_conj(up[p], v[be * 3 + c], sv[al * 3 + c]);
      p++;
    }
}

// trace = sum_{s2} row_value[iG][s2] * resG[s2][column_index[iG][s2]]; loopData[tid + V*iG] += trace (:110-120)
template <typename F> __device__ inline void trace_and_store(Cplx<F> *loop, const Cplx<F> acc[16], int V, int site, bool overwrite = false) {
#pragma unroll
  for (int iG = 0; iG < 16; iG++) {
    Cplx<F> t{F(0), F(0)};
#pragma unroll
    for (int s2 = 0; s2 < 4; s2++) add_phase(t, kGammaPhase[iG][s2], acc[s2 * 4 + kGammaColumn[iG][s2]]);
    Cplx<F> *out = loop + (int64_t)V * iG + site;
    Cplx<F> o = overwrite ? Cplx<F>{F(0), F(0)} : *out;  // overwrite: the slot holds nothing yet (no memset, no read)
    o.re += t.re;
    o.im += t.im;
    *out = o;
  }
}

// the same for the gamma channels [G0, G1) only (the tile kernel splits the 16 channels over the two lane halves)
template <typename F, int G0, int G1> __device__ inline void trace_and_store_range(Cplx<F> *loop, const Cplx<F> acc[16], int V, int site, bool overwrite = false) {
#pragma unroll
  for (int iG = G0; iG < G1; iG++) {
    Cplx<F> t{F(0), F(0)};
#pragma unroll
    for (int s2 = 0; s2 < 4; s2++) add_phase(t, kGammaPhase[iG][s2], acc[s2 * 4 + kGammaColumn[iG][s2]]);
    Cplx<F> *out = loop + (int64_t)V * iG + site;
    Cplx<F> o = overwrite ? Cplx<F>{F(0), F(0)} : *out;  // overwrite: the slot holds nothing yet (no memset, no read)
    o.re += t.re;
    o.im += t.im;
    *out = o;
  }
}

// the four gamma traces G0 .. G0 + 3 of a colour-traced spin matrix, returned instead of stored
template <typename F, int G0> __device__ inline void traces_range(Cplx<F> out[4], const Cplx<F> acc[16]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    Cplx<F> t{F(0), F(0)};
#pragma unroll
    for (int s2 = 0; s2 < 4; s2++) add_phase(t, kGammaPhase[G0 + i][s2], acc[s2 * 4 + kGammaColumn[G0 + i][s2]]);
    out[i] = t;
  }
}

// ---- workgroup order -------------------------------------------------------------------------------------------
// Workgroups are dealt round-robin over the 8 XCDs.  Where neighbouring blocks of a grid share cache lines (x-adjacent aggregates
// of the MG kernels), XCD k walks the k-th contiguous eighth of the blocks instead, so the sharers run side by side on one L2.
__device__ inline int xcd_contiguous_block(int blk, int nblk) {
  if (nblk & 7) return blk;
  return (blk & 7) * (nblk >> 3) + (blk >> 3);
}

// ---- QUDA even-odd index helpers (upstream QUDA index_helper.cuh) --------------
__host__ __device__ inline void get_coords(int c[4], int x_cb, const int X[4], int parity) {
  const int za = x_cb / (X[0] >> 1);
  const int zb = za / X[1];
  c[1] = za - zb * X[1];
  c[3] = zb / X[2];
  c[2] = zb - c[3] * X[2];
  const int x1odd = (c[1] + c[2] + c[3] + parity) & 1;
  c[0] = 2 * x_cb + x1odd - za * X[0];
}
__host__ __device__ inline int lex_index(const int c[4], const int X[4]) {
  return ((c[3] * X[2] + c[2]) * X[1] + c[1]) * X[0] + c[0];
}
// linkIndexShift(x, dx, X) with y[i] = (x[i] + dx[i] + X[i]) % X[i]
__host__ __device__ inline int link_index_shift(const int c[4], const int dx[4], const int X[4]) {
  int y[4];
#pragma unroll
  for (int i = 0; i < 4; i++) y[i] = (c[i] + dx[i] + X[i]) % X[i];
  return lex_index(y, X) >> 1;
}
// ghostFaceIndex<bnd>(x, X, dim, nFace = 1) on the face: the leading term vanishes
__host__ __device__ inline int ghost_face_index_on_face(const int c[4], const int X[4], int dim) {
  int idx;
  switch (dim) {
  case 0: idx = (c[3] * X[2] + c[2]) * X[1] + c[1]; break;
  case 1: idx = (c[3] * X[2] + c[2]) * X[0] + c[0]; break;
  case 2: idx = (c[3] * X[1] + c[1]) * X[0] + c[0]; break;
  default: idx = (c[2] * X[1] + c[1]) * X[0] + c[0]; break;
  }
  return idx >> 1;
}

// ---- native field accessors -------------------------------------------------------------------------
// Spinor body (or ghost zone) in FLOAT2 / FLOAT4 order; see MugiqHipSpinorField in mugiq_hip.h.
template <typename F, int ORDER> struct SpinorView {
  F *base;
  int stride;
  int64_t parity_offset;  // complex elements

  __device__ inline void load(Cplx<F> v[12], int parity, int x_cb) const {
    const Cplx<F> *p = reinterpret_cast<const Cplx<F> *>(base) + parity * parity_offset;
    if constexpr (ORDER == 2) {
#pragma unroll
      for (int k = 0; k < 12; k++) v[k] = p[(int64_t)k * stride + x_cb];
    } else {
      struct alignas(4 * sizeof(F)) Pair {
        Cplx<F> a, b;
      };
      const Pair *q = reinterpret_cast<const Pair *>(p);
#pragma unroll
      for (int j = 0; j < 6; j++) {
        Pair t = q[(int64_t)j * stride + x_cb];
        v[2 * j] = t.a;
        v[2 * j + 1] = t.b;
      }
    }
  }
  __device__ inline void store(const Cplx<F> v[12], int parity, int x_cb) const {
    Cplx<F> *p = reinterpret_cast<Cplx<F> *>(base) + parity * parity_offset;
    if constexpr (ORDER == 2) {
#pragma unroll
      for (int k = 0; k < 12; k++) p[(int64_t)k * stride + x_cb] = v[k];
    } else {
      struct alignas(4 * sizeof(F)) Pair {
        Cplx<F> a, b;
      };
      Pair *q = reinterpret_cast<Pair *>(p);
#pragma unroll
      for (int j = 0; j < 6; j++) q[(int64_t)j * stride + x_cb] = Pair{v[2 * j], v[2 * j + 1]};
    }
  }
};

template <typename F, int ORDER> inline SpinorView<F, ORDER> make_view(const MugiqHipSpinorField &f) {
  return SpinorView<F, ORDER>{static_cast<F *>(f.data), f.stride, f.parity_offset};
}
template <typename F, int ORDER> inline SpinorView<F, ORDER> make_ghost_view(void *zone, int faceCB) {
  return SpinorView<F, ORDER>{static_cast<F *>(zone), faceCB, (int64_t)12 * faceCB};
}

// Gauge field in native FLOAT2 order, 18 reals per link (reconstruct NO).
template <typename F> struct GaugeView {
  const F *base;
  int stride;
  int64_t parity_offset;
  __device__ inline void load(Cplx<F> u[9], int dir, int parity, int x_cb) const {
    const Cplx<F> *p = reinterpret_cast<const Cplx<F> *>(base) + parity * parity_offset + (int64_t)dir * 9 * stride + x_cb;
#pragma unroll
    for (int i = 0; i < 9; i++) u[i] = p[(int64_t)i * stride];
  }
};

int validate_spinor(const MugiqHipSpinorField *f, const char *who, const char *name);
// comm_dim_partitioned(d) (include/contract_util.cuh:89): more than one rank along d, or the partitioned code path forced
// on an axis of extent 1 (the rank is then its own neighbour; QUDA's comm_dim_partitioned_set)
inline bool comm_partitioned(const MugiqHipComm *c, int d) { return c != nullptr && (c->grid[d] > 1 || c->partitioned[d] != 0); }
bool same_geometry(const MugiqHipSpinorField &a, const MugiqHipSpinorField &b);
// [first, last) byte range a spinor's kernels may touch
inline void spinor_span(const MugiqHipSpinorField &f, uintptr_t *a, uintptr_t *b) {
  *a = reinterpret_cast<uintptr_t>(f.data);
  *b = *a + (uintptr_t)(f.parity_offset + (int64_t)12 * f.stride) * 2 * f.precision;
}
// no a_i shares a byte with a b_j (b NULL: with an a_j, j < i).  identicalOk: a_i may be b_i itself, body on body.  The message names
// the two sets and ends in `note`
inline int check_disjoint(const MugiqHipSpinorField *a, int na, const char *aName, const MugiqHipSpinorField *b, int nb, const char *bName,
                          const char *who, bool identicalOk = false, const char *note = "") {
  for (int i = 0; i < na; i++) {
    uintptr_t a0, a1;
    spinor_span(a[i], &a0, &a1);
    for (int j = 0; j < (b ? nb : i); j++) {
      const MugiqHipSpinorField &o = b ? b[j] : a[j];
      uintptr_t b0, b1;
      spinor_span(o, &b0, &b1);
      MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1) || (identicalOk && j == i && a[i].data == o.data), "%s: %s vector %d overlaps %s vector %d%s", who, aName, i,
                    bName, j, note);
    }
  }
  return MUGIQ_HIP_SUCCESS;
}
// [first, last) bytes of a coarse field's body (csrc/coarse_op.hip, csrc/coarse_eig.hip)
inline void coarse_span(const MugiqHipCoarseField &f, uintptr_t *a, uintptr_t *b) {
  *a = reinterpret_cast<uintptr_t>(f.data);
  *b = *a + (uintptr_t)(f.parity_offset + (int64_t)2 * f.nColor * f.stride) * 2 * f.precision;
}
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }  // sub-buffers of the per-stream arenas

}  // namespace mugiq
