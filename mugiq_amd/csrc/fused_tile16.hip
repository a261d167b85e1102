// LDS-tiled fused displaced contraction with 16-line items: the tile of csrc/fused_tile.hip cut into 16-line pieces.
//
// The unit of work ("item") is one (position, slot) pair on 16 lines = 32 lanes (two spin halves), two items per wave:
//   * row tile (mu = x): positions are 16-entry pieces of whole x rows, lcm(16, X0/2)/16 per parity -- at X0 = 48 two rows =
//     three pieces per parity, 6 positions x 3 slots = 18 items = 9 waves, every lane busy (the 32-line positions of
//     csrc/fused_tile.hip hold one 24-entry row each there: a quarter of every wave idle);
//   * column tile (mu = y, z, t): 4 positions x 3 slots = 12 items = 6 waves, 2 x 21.5 KB of LDS, two workgroups per CU.
// Staging is by linear element index (element e of the [position][12][16] tile <-> thread e mod #threads), so any number of
// waves stages any tile.  Arithmetic, prefetch depth, barrier discipline and the ghost / wrap handling are those of
// csrc/fused_tile.hip: one text, csrc/vector_tile.h.  Which generation takes what is decided by measurement (tile16_admits in
// csrc/fused_form.cpp).
#include "vector_tile.h"

namespace mugiq {

// (kT16Cols, kT16MaxSlots, kT16MaxItems, kT16MaxPos, kT16Row: csrc/fused_form.h)
template <typename F, typename A> struct Tile16Args : VectorTileArgs<F, A, kT16MaxSlots> {
  Cplx<A> *loop;
  int64_t slot_stride;
  int tj;         // column tile: positions along mu per tile
  int npc;        // computed positions per tile (column: TJ; row: 2 m)
  int np;         // staged positions per tile (column: TJ + kmax; row: 2 m)
  int m;          // row tile: 16-entry pieces per parity
};

// PHL bounds the staging loads per lane and eigenvector (ceil(np * 192 / #threads)).
// GLDS (fp64 FLOAT2 storage; round 3): the tile goes global -> LDS directly into THREE buffers (MUGIQ_VT_PIPELINE_GLDS).  The staging index is
// already linear in the thread (element e <-> thread e mod #threads), which is the lane-linear image the transfer wants.
template <typename F, typename A, int ORDER, int DIR, int SIGN, int PHL, bool GLDS>
__device__ __forceinline__ void tile16_body(const Tile16Args<F, A> &a) {
  extern __shared__ __align__(16) unsigned char smem[];
  Cplx<F> *tileBase = reinterpret_cast<Cplx<F> *>(smem);  // 2 (GLDS: 3) x [PHL * #threads] (buffered over the eigenvectors)
  const int nthreads = blockDim.x;
  const size_t tileElems = (size_t)PHL * nthreads;        // padded: commits are unconditional
  const int t = threadIdx.x, lane = t & 63;
  const int col = lane & 15, half = (lane >> 4) & 1;
  const int item = 2 * (t >> 6) + (lane >> 5);
  const bool computes = item < a.npc * a.nslot;
  const int wpos = item % a.npc;  // this item's own position
  const int slot = computes ? item / a.npc : 0;
  const int k = a.k[slot];
  const int nElem = a.np * kT16Row;

  const int blk = xcd_contiguous_block(a.blockOrder);
  // ---- the tile.  Column tile: 16 lines along mu x TJ consecutive positions j0 .. j0 + TJ - 1 (csrc/vector_tile.h).  Row tile: m
  // 16-entry pieces of whole x rows per parity, position pp = parity | piece << 1; entry f = piece * 16 + col of the tile's run of
  // m * 16 checkerboard entries.
  int j0 = 0, tileBaseX = 0;
  ColumnLine ln = {0, 0, 0, true};
  if constexpr (DIR >= 1) {
    const int jt = a.jtBegin + blk % a.jtCount;
    j0 = jt * a.tj;
    ln = column_line<DIR>(a, (blk / a.jtCount) * kT16Cols + col);
  } else {
    tileBaseX = blk * (a.m * kT16Cols);
  }
  const Cplx<F> *ghostBase = reinterpret_cast<const Cplx<F> *>(a.ghost);

  // ---- staging: element e = (pp * 12 + comp) * 16 + c of the tile <-> thread e mod #threads (c == col: #threads is a
  // multiple of 16); where thread t commits its element i: e itself, surplus slots re-read an element of the last row (same value,
  // same place).  Source offset and "is a ghost layer" bit are fixed for the whole kernel
  auto commit_index = [&](int i) {
    const int e = t + nthreads * i;
    return e < nElem ? e : nElem - kT16Cols + col;
  };
  int soff[PHL];
  unsigned sghost = 0;
#pragma unroll
  for (int i = 0; i < PHL; i++) {
    const int e = commit_index(i);
    const int pp = e / kT16Row, comp = (e - pp * kT16Row) >> 4;
    if constexpr (DIR >= 1) {
      soff[i] = column_stage_offset<ORDER, DIR, SIGN>(a, ln, j0, pp, comp, 1u << i, sghost);
    } else {
      soff[i] = (int)((int64_t)(pp & 1) * a.parity_offset + comp_offset<ORDER>(comp, a.stride, tileBaseX + (pp >> 1) * kT16Cols + col));
    }
  }

  // ---- my site, and the LDS slots of my v(x) and of my shifted v(x +- k mu)
  TileItem it;
  int colS = col;
  if constexpr (DIR >= 1) {
    it = column_item<SIGN>(a, ln, j0, wpos, k);
  } else {
    const int ePR = a.X[0] >> 1;  // checkerboard entries per x row; the tile's run starts on a row boundary
    it.ppL = wpos;
    it.pmine = wpos & 1;
    const int f = (wpos >> 1) * kT16Cols + col;
    it.xmine = tileBaseX + f;
    int c[4];
    get_coords(c, it.xmine, a.X, it.pmine);
    int xs = c[0] + ((SIGN == MUGIQ_HIP_DISP_SIGN_PLUS) ? k : -k);
    xs %= a.X[0];
    if (xs < 0) xs += a.X[0];
    const int fs = (f / ePR) * ePR + (xs >> 1);  // same row, entry x' / 2; the parity flips for odd k
    it.ppS = ((fs >> 4) << 1) | (it.pmine ^ (k & 1));
    colS = fs & 15;
  }

  Cplx<A> Wr[9];
  load_path_link<F, A>(Wr, a.E[slot], it.pmine, it.xmine, a.volumeCB);
  Cplx<A> acc[8];  // acc[be*2 + a2], al = 2*half + a2
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i] = Cplx<A>{A(0), A(0)};

#define MUGIQ_T16_COMPUTE(tile_, s_)                                                                                   \
  {                                                                                                                    \
    const Cplx<F> *tile = tile_;                                                                                       \
    const A s = s_;                                                                                                    \
    if (computes)                                                                                                      \
      MUGIQ_VT_COMPUTE(kT16Cols, tile + (it.ppL * 12) * kT16Cols + col, tile + (it.ppS * 12 + half * 6) * kT16Cols + colS, s, false)       \
  }
  if constexpr (GLDS) {
    // transfer i of wave w: elements w * 64 + lane + #threads * i; every wave stages
    [[maybe_unused]] const int wave = __builtin_amdgcn_readfirstlane(t >> 6);  // (unused in the host pass)
    MUGIQ_VT_PIPELINE_GLDS(PHL, true, (size_t)wave * 64, nthreads, MUGIQ_T16_COMPUTE)
  } else {
    MUGIQ_VT_PIPELINE_REGISTERS(PHL, commit_index, MUGIQ_T16_COMPUTE)
  }
#undef MUGIQ_T16_COMPUTE
  // ---- epilogue: the two lane halves of an item hold the same 16 sites
  MUGIQ_VT_EXCHANGE_HALVES(16)
  if (computes && ln.active) MUGIQ_VT_STORE_TRACES(a.loop + (int64_t)slot * a.slot_stride, it.xmine + it.pmine * a.volumeCB)
}

// (the body behind a reference to the kernel's argument: written straight into the kernel, hipcc spills more in two row-tile instances)
template <typename F, typename A, int ORDER, int DIR, int SIGN, int PHL, bool GLDS>
__global__ __launch_bounds__(64 * 12) void tile16_displaced_contract_kernel(Tile16Args<F, A> a) {
  tile16_body<F, A, ORDER, DIR, SIGN, PHL, GLDS>(a);
}

// g: tile16_launch_geometry of this launch (csrc/fused_form.cpp)
template <typename F, typename A, int ORDER> static int launch_tile16(Tile16Args<F, A> a, int dir, int sign, const Tile16Launch &g, hipStream_t stream) {
  const unsigned nblocks = dir == 0 ? (unsigned)(a.volumeCB / (a.m * kT16Cols)) : (unsigned)(((a.numCols + kT16Cols - 1) / kT16Cols) * a.jtCount);
  a.blockOrder = g.block_order(nblocks);
  return dispatch_dir_sign(dir, sign, [&](auto D, auto S) -> int {
    constexpr int DIR = decltype(D)::value, SIGN = decltype(S)::value;
    auto launch = [&](auto kern) { return launch_vector_tile(kern, nblocks, g.waves, g.ldsBytes, stream, a); };
    // the instance that bounds the staging loads per lane; global -> LDS staging with three buffers (fp64 FLOAT2), else register
    // staging with two
    auto with_phl = [&](auto P) -> int {
      constexpr int PHL = decltype(P)::value;
      if constexpr (std::is_same<F, double>::value && ORDER == 2) {
        if (g.glds) return launch(tile16_displaced_contract_kernel<F, A, ORDER, DIR, SIGN, PHL, true>);
      }
      return launch(tile16_displaced_contract_kernel<F, A, ORDER, DIR, SIGN, PHL, false>);
    };
    return g.phlSel == 2 ? with_phl(std::integral_constant<int, 2>()) : g.phlSel == 4 ? with_phl(std::integral_constant<int, 4>())
                                                                                      : with_phl(std::integral_constant<int, 8>());
  });
}

template <typename F, typename A, int ORDER>
int tile16_entry(const FusedForm &form, void *loop_d, const MugiqHipSpinorField *ev, const double *sigma, int nVec, const void *const *E_d,
                 const int *kvals, int nK, int sign, const void *ghost_d, int layers, int region, hipStream_t stream) {
  const int dir = form.dir;
  Tile16Args<F, A> a;
  int st = fill_vector_tile_args(a, form, ev, sigma, nVec, ghost_d, layers, region, stream);
  if (st) return st;
  a.slot_stride = (int64_t)16 * 2 * ev[0].volumeCB;
  a.tj = form.sw.tile16Tj;
  const int nJT = dir == 0 ? 1 : ev[0].X[dir] / a.tj;
  for (int k0 = 0; k0 < nK; k0 += form.slotsPerLaunch) {
    fill_vector_tile_slots(a, E_d, kvals, k0, std::min(nK - k0, form.slotsPerLaunch));
    a.loop = static_cast<Cplx<A> *>(loop_d) + (int64_t)k0 * a.slot_stride;
    const Tile16Launch g = tile16_launch_geometry(form, a.nslot, a.kmax);
    a.m = g.m;
    a.npc = g.npc;
    a.np = g.np;
    tile_range(region, form.partitioned, sign, nJT, a.kmax, a.tj, a.jtBegin, a.jtCount);
    if (a.jtCount > 0) {
      st = launch_tile16<F, A, ORDER>(a, dir, sign, g, stream);
      if (st) return st;
    }
  }
  return MUGIQ_HIP_SUCCESS;
}

#define MUGIQ_T16_INST(F, A, O)                                                                                                    \
  template int tile16_entry<F, A, O>(const FusedForm &, void *, const MugiqHipSpinorField *, const double *, int, const void *const *, const int *, \
                                     int, int, const void *, int, int, hipStream_t);
MUGIQ_T16_INST(double, double, 2)
MUGIQ_T16_INST(double, double, 4)
MUGIQ_T16_INST(float, float, 2)
MUGIQ_T16_INST(float, float, 4)
MUGIQ_T16_INST(float, double, 2)
MUGIQ_T16_INST(float, double, 4)
#undef MUGIQ_T16_INST

}  // namespace mugiq
