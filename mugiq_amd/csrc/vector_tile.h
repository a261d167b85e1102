// What the two vector tiles of the fused displaced contraction share (csrc/fused_tile.hip: 32 lines per workgroup, one wave per
// (position, slot); csrc/fused_tile16.hip: 16-line items, two per wave): the geometry of a column tile, the load of W_k, the arithmetic
// of one eigenvector on a tile buffer, the two eigenvector pipelines (staged through registers | global -> LDS), the epilogue, and on the
// host the common kernel arguments, the launch and the (direction, sign) dispatch.  Device and launch code: included by those two
// files only.  A generation keeps what is its own: the tile and item maps, the staging index, the LDS image, the row tiles, the
// carried slot and the slot tables; it hands a pipeline the one thing that differs (where a staging slot commits | where a transfer
// lands) and the arithmetic on its own LDS image.
#pragma once
#include "internal.h"

#include <algorithm>
#include <type_traits>

namespace mugiq {

// ---- kernel arguments of both generations (NS: slots per launch), filled by fill_vector_tile_args / fill_vector_tile_slots
template <typename F, typename A, int NS> struct VectorTileArgs {
  typedef F Storage;
  typedef A Accum;
  const void *const *L;
  const A *inv_sigma;
  int nVec;
  int X[4];
  int volumeCB;
  int stride;
  int64_t parity_offset;
  const F *E[NS];  // path links W_k of every slot; NULL = the identity (k = 0)
  int k[NS];
  int nslot;
  int kmax;
  int partitioned;
  const F *ghost;
  int64_t ghost_vec_stride;
  int faceCB;
  int strideMu;   // x_cb distance of one step along DIR
  int H;          // volumeCB / (X[DIR] * strideMu)
  int numCols;    // V / X[DIR]
  int jtBegin;    // column tile: tiles along mu handled by this launch: [jtBegin, jtBegin + jtCount)
  int jtCount;
  int blockOrder; // workgroup -> tile map: bit 1 XCD-contiguous (xcd_contiguous_block); bit 0: the 32-line kernel's own
  int overwrite;  // store instead of accumulate (MUGIQ_HIP_REGION_OVERWRITE)
};

// ---- helpers
// complex-element offset of component `comp` at checkerboard index idx inside one parity block of a field / ghost zone
template <int ORDER> __device__ inline int64_t comp_offset(int comp, int64_t stride, int64_t idx) {
  if constexpr (ORDER == 2) return (int64_t)comp * stride + idx;
  else return ((int64_t)(comp >> 1) * stride + idx) * 2 + (comp & 1);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() lowers to `s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier`,
// i.e. it also drains every global load in flight -- which would serialise the register prefetch of the next
// eigenvectors behind each barrier.  The stage registers are guarded by the compiler's own counted vmcnt waits.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// the tile of this workgroup.  XCD-contiguous order (blockOrder & 2): workgroups are dealt round-robin over the 8 XCDs
__device__ __forceinline__ int xcd_contiguous_block(int blockOrder) {
  int blk = blockIdx.x;
  if (blockOrder & 2) {
    const int per = gridDim.x >> 3;
    blk = (blk & 7) * per + (blk >> 3);
  }
  return blk;
}

// ---- column tile (DIR >= 1): lines along mu x consecutive positions j0 .. on them; staged position pp <-> coordinate j = j0 + pp
// (sign +) | j0 - kmax + pp (sign -), parity alternating with j, x_cb = base + j * strideMu
struct ColumnLine {
  int p0, base, faceIdx;  // parity and x_cb of the line's j = 0 site, its index on the face
  bool active;
};
// line cid of the lattice
template <int DIR, typename Args> __device__ __forceinline__ ColumnLine column_line(const Args &a, int cid) {
  ColumnLine ln;
  ln.active = cid < a.numCols;
  if (!ln.active) cid = a.numCols - 1;  // surplus lanes shadow the last line (valid addresses, result dropped)
  const int colsPerParity = a.H * a.strideMu;
  ln.p0 = cid / colsPerParity;
  const int rem = cid - ln.p0 * colsPerParity;
  const int hi = rem / a.strideMu;
  const int lo = rem - hi * a.strideMu;
  ln.base = hi * (a.X[DIR] * a.strideMu) + lo;  // x_cb of the line's j = 0 site (parity p0)
  int c0[4];
  get_coords(c0, ln.base, a.X, ln.p0);          // c0[DIR] == 0
  ln.faceIdx = ghost_face_index_on_face(c0, a.X, DIR);
  return ln;
}
// source of component comp of staged position pp on line ln: the element offset; `bit` is set in sghost where it counts from the ghost
// zone (positions beyond the local extent come from the ghost layers (partitioned) or wrap around (periodic))
template <int ORDER, int DIR, int SIGN, typename Args>
__device__ __forceinline__ int column_stage_offset(const Args &a, const ColumnLine &ln, int j0, int pp, int comp, unsigned bit, unsigned &sghost) {
  const int J = a.X[DIR];
  int j = (SIGN == MUGIQ_HIP_DISP_SIGN_PLUS) ? j0 + pp : j0 - a.kmax + pp;
  const int par = ln.p0 ^ (j & 1);
  if ((j < 0 || j >= J) && a.partitioned) {
    const int layer = (j >= J) ? j - J : -j - 1;
    sghost |= bit;
    return (int)((int64_t)layer * 24 * a.faceCB + (int64_t)par * 12 * a.faceCB + comp_offset<ORDER>(comp, a.faceCB, ln.faceIdx));
  }
  j = j < 0 ? j + J : (j >= J ? j - J : j);
  return (int)((int64_t)par * a.parity_offset + comp_offset<ORDER>(comp, a.stride, ln.base + j * a.strideMu));
}
// the site of an item and the staged positions of its v(x) and of its shifted v(x +- k mu)
struct TileItem {
  int pmine, xmine, ppL, ppS;
};
template <int SIGN, typename Args> __device__ __forceinline__ TileItem column_item(const Args &a, const ColumnLine &ln, int j0, int wpos, int k) {
  TileItem it;
  it.ppL = (SIGN == MUGIQ_HIP_DISP_SIGN_PLUS) ? wpos : a.kmax + wpos;
  it.ppS = (SIGN == MUGIQ_HIP_DISP_SIGN_PLUS) ? wpos + k : a.kmax + wpos - k;
  const int jmine = j0 + wpos;
  it.pmine = ln.p0 ^ (jmine & 1);
  it.xmine = ln.base + jmine * a.strideMu;
  return it;
}

// ---- W_k(x) of this lane's site (both lane halves hold the same 3x3): in VGPRs.  It used to sit in LDS (9 of the 27 LDS
// reads per eigenvector) because the registers were short; fp32 storage has the room (stage registers half as wide:
// -7 % / -9 % per entry), fp64 gets it by prefetching two eigenvectors ahead instead of three (the kernel is bound by
// vector issue, not by memory latency: -3.6 % column, -2 % row tile; three-deep AND W in registers spills, +35 %).
template <typename F, typename A> __device__ __forceinline__ void load_path_link(Cplx<A> (&Wr)[9], const F *E, int pmine, int xmine, int volumeCB) {
  const Cplx<F> *e = reinterpret_cast<const Cplx<F> *>(E) + (int64_t)pmine * 12 * volumeCB + xmine;
#pragma unroll
  for (int j = 0; j < 3; j++)
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const Cplx<F> t = e[(int64_t)(j * 3 + i) * volumeCB];
      Wr[i * 3 + j] = Cplx<A>{(A)t.re, (A)t.im};
    }
}

// ---- the arithmetic of one eigenvector (scaled by s_) on a tile buffer: tl_ = component 0 of this item's v(x), ts_ = the first
// component of its two spins (2*half, 2*half + 1) of the shifted vector, CS_ = the distance between components in the LDS image.
// Expects acc[be*2 + a2], al = 2*half + a2, and Wr in scope.  unitW_: W = 1 (a wave-uniform branch; the 16-line kernel, which
// carries no such slot, passes false).  A macro like the pipelines below, and for their reason: as a __forceinline__ function the same
// statements cost the 12-wave global -> LDS form two VGPRs more, 130, past the 128 of four waves per SIMD.
#define MUGIQ_VT_COMPUTE(CS_, tl_, ts_, s_, unitW_)                                                                    \
  {                                                                                                                    \
    const Cplx<F> *tl = tl_;                                                                                           \
    const Cplx<F> *ts = ts_;                                                                                           \
    /* t[a2] = s * W * psi[2*half + a2]: each W element and each psi element is read from LDS once */                  \
    Cplx<A> t0[3], t1[3];                                                                                              \
    if (unitW_) { /* the carried ultra-local slot: W = 1 (wave-uniform branch) */                                      \
      _Pragma("unroll") for (int j = 0; j < 3; j++) {                                                                  \
        const Cplx<F> w0 = ts[j * CS_], w1 = ts[(3 + j) * CS_];                                                        \
        t0[j] = Cplx<A>{(A)w0.re, (A)w0.im};                                                                           \
        t1[j] = Cplx<A>{(A)w1.re, (A)w1.im};                                                                           \
      }                                                                                                                \
    } else {                                                                                                           \
      _Pragma("unroll") for (int i = 0; i < 3; i++) t0[i] = t1[i] = Cplx<A>{A(0), A(0)};                               \
      _Pragma("unroll") for (int j = 0; j < 3; j++) {                                                                  \
        const Cplx<F> w0 = ts[j * CS_], w1 = ts[(3 + j) * CS_];                                                        \
        const Cplx<A> p0j{(A)w0.re, (A)w0.im}, p1j{(A)w1.re, (A)w1.im};                                                \
        _Pragma("unroll") for (int i = 0; i < 3; i++) {                                                                \
          const Cplx<A> w = Wr[i * 3 + j];                                                                             \
          cmadd(t0[i], w, p0j);                                                                                        \
          cmadd(t1[i], w, p1j);                                                                                        \
        }                                                                                                              \
      }                                                                                                                \
    }                                                                                                                  \
    _Pragma("unroll") for (int i = 0; i < 3; i++) {                                                                    \
      t0[i] = Cplx<A>{s_ * t0[i].re, s_ * t0[i].im};                                                                   \
      t1[i] = Cplx<A>{s_ * t1[i].re, s_ * t1[i].im};                                                                   \
    }                                                                                                                  \
    _Pragma("unroll") for (int be = 0; be < 4; be++) {                                                                 \
      if (be == 2) __builtin_amdgcn_sched_barrier(0); /* bound how many LDS reads the scheduler hoists (VGPRs) */      \
      _Pragma("unroll") for (int c = 0; c < 3; c++) {                                                                  \
        const Cplx<F> u = tl[(be * 3 + c) * CS_];                                                                      \
        const Cplx<A> lv{(A)u.re, (A)u.im};                                                                            \
        cmadd_conj(acc[be * 2 + 0], lv, t0[c]);                                                                        \
        cmadd_conj(acc[be * 2 + 1], lv, t1[c]);                                                                        \
      }                                                                                                                \
    }                                                                                                                  \
  }

// ---- the pipelines over the eigenvectors: macros, expanded once in each kernel.  (As __forceinline__ templates that take the
// generation's part as lambdas they are the same statements, but hipcc allocates the kernels differently: ten instances came out
// with more scratch or a lower occupancy bound, among them the 12-wave global -> LDS form at 130 instead of 128 VGPRs.)
// They expect in scope: the kernel arguments `a`; F, A; soff[i] / bit i of sghost, the source of staging slot (transfer) i of this
// thread -- element offset and "counts from the ghost zone" -- fixed for the whole kernel, every slot with a valid source (surplus ones
// re-read); ghostBase; tileBase / tileElems, the tile buffers in LDS.  COMPUTE(tile, s): the generation's arithmetic of one eigenvector
// on buffer `tile` (MUGIQ_VT_COMPUTE on its LDS image).
#define MUGIQ_VT_BODY(n_) static_cast<const Cplx<F> *>(as_constant(a.L)[n_])
#define MUGIQ_VT_SIGMA(n_) as_constant(a.inv_sigma)[n_]

// Staged through registers, two tile buffers; PH_ staging slots per thread, COMMIT_AT(i): where slot i goes inside a tile buffer.
//
// Three eigenvectors in flight ahead of the one being consumed (fp64 storage: two, see load_path_link).  Diagnostic builds on MI355X
// (tools/probes/fused_tile_probes.patch; 48.48.24.24 fp64, 100 eigenvectors, 10.0 ms per entry): staging only 5.9 ms, compute only
// 7.0 ms (6.9 ms without the barrier); SQ counters: the VALU pipe of a SIMD is ~64 % busy, 82 % of its instructions are the FMAs of the
// mathematics -- the kernel is bound by vector issue, not by HBM or LDS.  Tried without gain: 6-deep prefetch for
// fp32 storage (25 % slower), a pair-wise LDS layout so that fp32 reads are ds_read_b128 instead of ds_read2_b64 (no
// change), column groups as the fastest workgroup index (4 % slower).
//
// fetch this thread's share of eigenvector n_ (body: its field)
#define MUGIQ_VT_FETCH(n_, stage, PH_) MUGIQ_VT_FETCH_AT(MUGIQ_VT_BODY(n_), n_, stage, PH_)
#define MUGIQ_VT_FETCH_AT(bodyExpr_, n_, stage, PH_)                                                                   \
  {                                                                                                                    \
    const Cplx<F> *body_ = bodyExpr_;                                                                                  \
    const Cplx<F> *gh_ = ghostBase + (int64_t)(n_)*a.ghost_vec_stride;                                                 \
    _Pragma("unroll") for (int i = 0; i < PH_; i++) { /* unconditional: every lane and slot has a valid source */      \
      const Cplx<F> *ptr_ = (((sghost >> i) & 1u) ? gh_ : body_) + soff[i];                                            \
      stage[i] = *as_global(reinterpret_cast<const vec2 *>(ptr_));                                                     \
    }                                                                                                                  \
  }
// One step: eigenvector n_ is in LDS buffer n_ % 2; `stage` holds eigenvector n_+1 (fetched kDepth steps ago).
// Commit n_+1 into the other buffer (everyone finished reading it before the barrier that ended the previous step),
// refill `stage` with n_ + kDepth + 1, consume n_, one barrier.  (Little's law: with one workgroup per CU the bytes in flight
// are what the stage registers hold -- 3 x 42 KB per CU sustains ~6 TB/s at ~4 us loaded latency, 2 x 42 KB does not.)
#define MUGIQ_VT_STEP(n_, stage, GUARD, PH_, COMMIT_AT, COMPUTE)                                                       \
  {                                                                                                                    \
    const A sNow = sigPre;                                                                                             \
    const Cplx<F> *bodyNow = bodyPre;                                                                                  \
    { /* table look-ups of the NEXT step, issued first: they complete while this step waits for its staged loads, and  \
         being scalar loads in flight they would otherwise turn the first LDS wait of the arithmetic into lgkmcnt(0) */ \
      const int nb_ = (n_) + kDepth + 2 < a.nVec ? (n_) + kDepth + 2 : a.nVec - 1, ns_ = (n_) + 1 < a.nVec ? (n_) + 1 : a.nVec - 1; \
      bodyPre = MUGIQ_VT_BODY(nb_);                                                                                    \
      sigPre = MUGIQ_VT_SIGMA(ns_);                                                                                    \
    }                                                                                                                  \
    __builtin_amdgcn_sched_barrier(0); /* keep them first */                                                           \
    if (GUARD == 0 || (n_) + 1 < a.nVec) {                                                                             \
      Cplx<F> *nxt = tileBase + (size_t)(((n_) + 1) & 1) * tileElems;                                                  \
      _Pragma("unroll") for (int i = 0; i < PH_; i++) nxt[COMMIT_AT(i)] = Cplx<F>{stage[i].x, stage[i].y};             \
    }                                                                                                                  \
    if (GUARD == 0 || (n_) + kDepth + 1 < a.nVec) MUGIQ_VT_FETCH_AT(bodyNow, (n_) + kDepth + 1, stage, PH_)            \
    COMPUTE(tileBase + (size_t)((n_) & 1) * tileElems, sNow)                                                           \
    lds_barrier();                                                                                                     \
  }
#define MUGIQ_VT_PIPELINE_REGISTERS(PH_, COMMIT_AT, COMPUTE)                                                           \
  {                                                                                                                    \
    typedef F vec2 __attribute__((ext_vector_type(2)));                                                                \
    constexpr int kDepth = sizeof(F) == 8 ? 2 : 3; /* eigenvectors in flight ahead of the one being consumed */        \
    vec2 stageA[PH_], stageB[PH_], stageC[PH_];                                                                        \
    /* prologue: eigenvector 0 -> LDS buffer 0; eigenvectors 1, 2 (, 3) in flight in stageA / stageB (/ stageC) */     \
    MUGIQ_VT_FETCH(0, stageC, PH_)                                                                                     \
    _Pragma("unroll") for (int i = 0; i < PH_; i++) tileBase[COMMIT_AT(i)] = Cplx<F>{stageC[i].x, stageC[i].y};        \
    /* unconditional (clamped) so that the steady-state loop is entered with a KNOWN number of loads in flight: with   \
       conditional prologue loads hipcc's wait-count pass waited for vmcnt(0) at the first commit of every loop        \
       iteration, i.e. for the loads issued one step earlier -- the three-deep prefetch was in effect one deep */      \
    {                                                                                                                  \
      const int last = a.nVec - 1;                                                                                     \
      MUGIQ_VT_FETCH((1 < last ? 1 : last), stageA, PH_)                                                               \
      MUGIQ_VT_FETCH((2 < last ? 2 : last), stageB, PH_)                                                               \
      if constexpr (kDepth == 3) MUGIQ_VT_FETCH((3 < last ? 3 : last), stageC, PH_)                                    \
    }                                                                                                                  \
    const Cplx<F> *bodyPre = MUGIQ_VT_BODY(a.nVec > kDepth + 1 ? kDepth + 1 : a.nVec - 1);                             \
    A sigPre = MUGIQ_VT_SIGMA(0);                                                                                      \
    lds_barrier();                                                                                                     \
    /* steady state without any data-dependent branch (hipcc's wait-count pass turns every conditional load into a     \
       conservative `vmcnt(0)`, which would serialise the prefetch), then a guarded tail */                            \
    int n = 0;                                                                                                         \
    for (; n + 2 * kDepth < a.nVec; n += kDepth) {                                                                     \
      MUGIQ_VT_STEP(n, stageA, 0, PH_, COMMIT_AT, COMPUTE)                                                             \
      MUGIQ_VT_STEP(n + 1, stageB, 0, PH_, COMMIT_AT, COMPUTE)                                                         \
      if constexpr (kDepth == 3) MUGIQ_VT_STEP(n + 2, stageC, 0, PH_, COMMIT_AT, COMPUTE)                              \
    }                                                                                                                  \
    for (; n < a.nVec; n += kDepth) {                                                                                  \
      MUGIQ_VT_STEP(n, stageA, 1, PH_, COMMIT_AT, COMPUTE)                                                             \
      if (n + 1 < a.nVec) MUGIQ_VT_STEP(n + 1, stageB, 1, PH_, COMMIT_AT, COMPUTE)                                     \
      if constexpr (kDepth == 3)                                                                                       \
        if (n + 2 < a.nVec) MUGIQ_VT_STEP(n + 2, stageC, 1, PH_, COMMIT_AT, COMPUTE)                                   \
    }                                                                                                                  \
  }

// Global -> LDS directly (global_load_lds_dwordx4: no stage registers, no ds_write pass) into THREE tile buffers -- one consumed, two
// in flight.  Per eigenvector a thread issues PH_ transfers of 64 x 16 bytes per wave, which land lane-linear: transfer i of this wave
// starts at element LAND0 + i * LAND_STRIDE of a tile buffer (wave-uniform); STAGES: this wave takes part in the staging.
#if defined(__HIP_DEVICE_COMPILE__)  // (global_load_lds is a device-only builtin: the host pass of hipcc must not see it)
// this lane's share of eigenvector n_ -> tile buffer buf_
#define MUGIQ_VT_GLDS(bodyExpr_, n_, buf_, PH_, STAGES, LAND0, LAND_STRIDE)                                            \
  {                                                                                                                    \
    const Cplx<F> *body_ = bodyExpr_;                                                                                  \
    const Cplx<F> *gh_ = ghostBase + (int64_t)(n_)*a.ghost_vec_stride;                                                 \
    Cplx<F> *dst_ = (buf_) + LAND0;                                                                                    \
    if (STAGES) {                                                                                                      \
    _Pragma("unroll") for (int i = 0; i < PH_; i++) {                                                                  \
      const Cplx<F> *ptr_ = (((sghost >> i) & 1u) ? gh_ : body_) + soff[i];                                            \
      __builtin_amdgcn_global_load_lds(as_global(reinterpret_cast<const vec2 *>(ptr_)),                                \
                                       (lds_void *)(dst_ + (size_t)i * LAND_STRIDE), 16, 0, 0);                        \
    }                                                                                                                  \
    }                                                                                                                  \
  }
// One step: eigenvector n_ lands in buffer cur_ (own share: counted vmcnt wait; everybody's: the barrier, which also
// says that nobody reads buffer nxt2_ = the one consumed in the previous step any more); eigenvector n_+2 is sent
// there, n_+1 stays in flight, n_ is consumed.  One barrier per step, no register staging, no ds_write pass.
#define MUGIQ_VT_GSTEP(n_, cur_, nxt2_, STEADY, PH_, STAGES, LAND0, LAND_STRIDE, COMPUTE)                              \
  {                                                                                                                    \
    const A sNow = sigPre;                                                                                             \
    const Cplx<F> *bodyNow = bodyPre;                                                                                  \
    if (STEADY || (n_) + 1 < a.nVec) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PH_) : "memory");                        \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                              \
    lds_barrier();                                                                                                     \
    if (STEADY || (n_) + 2 < a.nVec) MUGIQ_VT_GLDS(bodyNow, (n_) + 2, nxt2_, PH_, STAGES, LAND0, LAND_STRIDE)          \
    COMPUTE(cur_, sNow)                                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                                                 \
    { /* table look-ups of the next step (scalar loads: they complete under the tail of the arithmetic) */            \
      const int nb_ = (n_) + 3 < a.nVec ? (n_) + 3 : a.nVec - 1, ns_ = (n_) + 1 < a.nVec ? (n_) + 1 : a.nVec - 1;      \
      bodyPre = MUGIQ_VT_BODY(nb_);                                                                                    \
      sigPre = MUGIQ_VT_SIGMA(ns_);                                                                                    \
    }                                                                                                                  \
  }
#define MUGIQ_VT_PIPELINE_GLDS(PH_, STAGES, LAND0, LAND_STRIDE, COMPUTE)                                               \
  {                                                                                                                    \
    typedef F vec2 __attribute__((ext_vector_type(2)));                                                                \
    typedef __attribute__((address_space(3))) void lds_void;                                                           \
    Cplx<F> *const buf0 = tileBase, *const buf1 = tileBase + tileElems, *const buf2 = tileBase + 2 * tileElems;        \
    const int last = a.nVec - 1;                                                                                       \
    MUGIQ_VT_GLDS(MUGIQ_VT_BODY(0), 0, buf0, PH_, STAGES, LAND0, LAND_STRIDE)                                          \
    /* (unconditional: known count in flight) */                                                                       \
    MUGIQ_VT_GLDS(MUGIQ_VT_BODY((1 < last ? 1 : last)), (1 < last ? 1 : last), buf1, PH_, STAGES, LAND0, LAND_STRIDE)  \
    const Cplx<F> *bodyPre = MUGIQ_VT_BODY((2 < last ? 2 : last));                                                     \
    A sigPre = MUGIQ_VT_SIGMA(0);                                                                                      \
    int n = 0;                                                                                                         \
    for (; n + 4 < a.nVec; n += 3) {                                                                                   \
      MUGIQ_VT_GSTEP(n, buf0, buf2, 1, PH_, STAGES, LAND0, LAND_STRIDE, COMPUTE)                                       \
      MUGIQ_VT_GSTEP(n + 1, buf1, buf0, 1, PH_, STAGES, LAND0, LAND_STRIDE, COMPUTE)                                   \
      MUGIQ_VT_GSTEP(n + 2, buf2, buf1, 1, PH_, STAGES, LAND0, LAND_STRIDE, COMPUTE)                                   \
    }                                                                                                                  \
    for (; n < a.nVec; n += 3) { /* n % 3 == 0 here */                                                                 \
      MUGIQ_VT_GSTEP(n, buf0, buf2, 0, PH_, STAGES, LAND0, LAND_STRIDE, COMPUTE)                                       \
      if (n + 1 < a.nVec) MUGIQ_VT_GSTEP(n + 1, buf1, buf0, 0, PH_, STAGES, LAND0, LAND_STRIDE, COMPUTE)               \
      if (n + 2 < a.nVec) MUGIQ_VT_GSTEP(n + 2, buf2, buf1, 0, PH_, STAGES, LAND0, LAND_STRIDE, COMPUTE)               \
    }                                                                                                                  \
  }
#else
#define MUGIQ_VT_PIPELINE_GLDS(PH_, STAGES, LAND0, LAND_STRIDE, COMPUTE) {}
#endif

// ---- epilogue: the two lane halves of an item (DIST_ lanes apart) hold complementary halves of the 4x4 colour-traced spin matrix of
// the same sites.  MUGIQ_VT_EXCHANGE_HALVES declares full[16] and fills it by wavefront shuffles (lane ^ DIST_; expects acc and half);
// then each half takes 8 of the 16 gamma traces (MUGIQ_VT_STORE_TRACES: expects `a`, `half` and `full`).  Macros for the reason given
// at MUGIQ_VT_COMPUTE: as a function the exchange moved the scratch of six 16-line instances up.
#define MUGIQ_VT_EXCHANGE_HALVES(DIST_)                                                                                \
  Cplx<A> full[16];                                                                                                    \
  _Pragma("unroll") for (int be = 0; be < 4; be++)                                                                     \
    _Pragma("unroll") for (int a2 = 0; a2 < 2; a2++) {                                                                 \
      const Cplx<A> mine = acc[be * 2 + a2];                                                                           \
      Cplx<A> theirs;                                                                                                  \
      theirs.re = __shfl_xor(mine.re, DIST_);                                                                          \
      theirs.im = __shfl_xor(mine.im, DIST_);                                                                          \
      /* al = 2*half + a2 is mine, al = 2*(1-half) + a2 the partner's (selects keep the register indices static) */   \
      full[be * 4 + a2] = half == 0 ? mine : theirs;                                                                   \
      full[be * 4 + 2 + a2] = half == 0 ? theirs : mine;                                                               \
    }
#define MUGIQ_VT_STORE_TRACES(out_, siteIdx_)                                                                          \
  {                                                                                                                    \
    Cplx<A> *out = out_;                                                                                               \
    const int siteIdx = siteIdx_;                                                                                      \
    if (half == 0) trace_and_store_range<A, 0, 8>(out, full, 2 * a.volumeCB, siteIdx, a.overwrite != 0);               \
    else trace_and_store_range<A, 8, 16>(out, full, 2 * a.volumeCB, siteIdx, a.overwrite != 0);                        \
  }

// ---- host side
// everything of the arguments that does not depend on the launch; `region` comes back without its OVERWRITE bit
template <typename F, typename A, int NS>
int fill_vector_tile_args(VectorTileArgs<F, A, NS> &a, const FusedForm &form, const MugiqHipSpinorField *ev, const double *sigma, int nVec,
                          const void *ghost_d, int layers, int &region, hipStream_t stream) {
  const void *invSigma = nullptr;
  const int st = upload_vector_table(&a.L, &invSigma, ev, nullptr, sigma, nVec, (int)sizeof(F), (int)sizeof(A), stream);
  if (st) return st;
  a.inv_sigma = static_cast<const A *>(invSigma);
  a.nVec = nVec;
  for (int d = 0; d < 4; d++) a.X[d] = ev[0].X[d];
  a.volumeCB = ev[0].volumeCB;
  a.stride = ev[0].stride;
  a.parity_offset = ev[0].parity_offset;
  a.partitioned = form.partitioned;
  a.ghost = static_cast<const F *>(ghost_d);
  const LineGeometry lines = line_geometry(ev[0], form.dir, layers);
  a.faceCB = lines.faceCB;
  a.ghost_vec_stride = lines.ghost_vec_stride;
  a.strideMu = lines.strideMu;
  a.H = lines.H;
  a.numCols = lines.numCols;
  a.overwrite = (region & MUGIQ_HIP_REGION_OVERWRITE) ? 1 : 0;
  region &= 0xff;
  return MUGIQ_HIP_SUCCESS;
}
// the slots of one launch: lengths kvals[k0 .. k0 + nslot) with their links (surplus slots repeat the first: valid pointers)
template <typename F, typename A, int NS> void fill_vector_tile_slots(VectorTileArgs<F, A, NS> &a, const void *const *E_d, const int *kvals, int k0, int nslot) {
  a.nslot = nslot;
  a.kmax = 0;
  for (int s = 0; s < NS; s++) {
    const int i = k0 + (s < nslot ? s : 0);
    a.E[s] = static_cast<const F *>(E_d[i]);
    a.k[s] = kvals[i];
    if (s < nslot && kvals[i] > a.kmax) a.kmax = kvals[i];
  }
}

// a launch with the dynamic LDS it asks for: past 64 KB a kernel has to be told
template <typename Kernel, typename Args> int launch_vector_tile(Kernel kern, unsigned nblocks, int waves, size_t ldsBytes, hipStream_t stream, const Args &a) {
  if (ldsBytes > 64 * 1024)
    MUGIQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes));
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64 * waves), ldsBytes, stream, a);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

// fn(D, S) with the direction and the sign as compile-time constants: constexpr int DIR = decltype(D)::value
template <typename Fn> int dispatch_dir_sign(int dir, int sign, Fn &&fn) {
#define MUGIQ_VT_CASE(D, S) \
  case (D)*2 + (S): return fn(std::integral_constant<int, D>(), std::integral_constant<int, S>());
  switch (dir * 2 + sign) {
    MUGIQ_VT_CASE(0, 0) MUGIQ_VT_CASE(0, 1) MUGIQ_VT_CASE(1, 0) MUGIQ_VT_CASE(1, 1)
    MUGIQ_VT_CASE(2, 0) MUGIQ_VT_CASE(2, 1) MUGIQ_VT_CASE(3, 0) MUGIQ_VT_CASE(3, 1)
  }
#undef MUGIQ_VT_CASE
  return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "vector tile: direction %d, sign %d (internal)", dir, sign);
}

}  // namespace mugiq
