// LDS-tiled fused displaced contraction (second generation of csrc/fused.hip, same mathematics and same C entry point).
//
// Measured on MI355X (profiles/r01_fused_*): the first-generation kernel streams v_n(x) and v_n(x +- k mu) for every slot
// k from HBM/fabric -- 1 + nslots "units" of 24*B bytes per site and eigenvector -- and sits at the ~6 TB/s fabric limit
// with no cache reuse.  But v_n(x + k mu) IS v_n at another site of the same straight line along mu.  Here a workgroup owns
// 32 such lines ("columns": fixed other coordinates, consecutive coordinate j along mu, parity alternating with j) and TJ
// consecutive positions on them.  Per eigenvector it stages the TJ + Kmax positions it needs in LDS once (one component
// plane per wave, 512-byte runs over the lines), and every (position, slot) pair -- one wave each -- reads both its v_n(x)
// and its shifted v_n(x +- k mu) from LDS.  A workgroup requests (TJ + Kmax)/TJ units per site and eigenvector (TJ = 4,
// 3 slots: 1.75); with the XCD-contiguous workgroup order the Kmax halo positions are the core positions of the
// neighbouring tile on the same XCD and come out of its L2, so the HBM traffic is read-once (PMC: 27-28 GB per entry
// against 45 GB with the plain order, profiles/r02_pmc_extra_traffic.txt).  What bounds the kernel is fp64 issue at the
// clock the device grants under this mix of FMAs, LDS reads and loads (1.72-1.78 GHz, profiles/r02_kernel_clocks.txt).
// Staging: global -> LDS directly with three tile buffers (fp64 FLOAT2, <= 8 positions), otherwise through registers with
// two buffers; one LDS-only barrier per eigenvector either way.
// Positions beyond the local extent come from the ghost layers (partitioned) or wrap around (periodic), exactly as in
// the first-generation kernel.  Requirements: X[DIR] % TJ == 0, at most 3 slots per launch; DIR == 0 is the row tile
// (whole x-rows per workgroup, see the kernel; rows that do not fill 32 lanes go to csrc/fused_tile16.hip).
// The column geometry, the arithmetic, the two eigenvector pipelines and the epilogue are those of csrc/vector_tile.h, shared with the
// 16-line kernel; here: the tile and wave maps, the plane-per-wave staging, the LDS images, the row tile and the carried slot.
#include "vector_tile.h"

namespace mugiq {

// (kTileTJ, kTileMaxSlots, kTileCarry, kTileMaxPos, kTileCols: csrc/fused_form.h)
template <typename F, typename A> struct TileArgs : VectorTileArgs<F, A, kTileCarry> {
  Cplx<A> *out[kTileCarry];  // where every slot goes
};

// Workgroup = 12 waves over 32 lines.  Wave w <-> (position jj = w % TJ, slot = w / TJ); inside a wave lanes 0-31 and
// 32-63 hold the SAME 32 lines and split the right-hand spin index (al in {0,1} | {2,3}), so a lane carries 8 of the 16
// accumulators -- at three waves per SIMD a lane has ~168 VGPRs, which 16 fp64 accumulators + W + the prefetch
// registers do not fit into.  For staging, wave w owns plane w (component 3*spin + colour): its two lane halves fetch
// alternate positions (32 lanes x 16 B = one 512-byte run each).  PH bounds the positions staged per lane.
//
// GLDS (fp64 FLOAT2 storage, column tiles of at most 8 positions): the staged positions go global -> LDS directly
// (MUGIQ_VT_PIPELINE_GLDS) into THREE tile buffers.  The transfer wants a lane-linear LDS image, so a buffer is
// [position pair][12][position & 1][32]: the two lane halves of an instruction (alternate positions, 512 bytes each) land
// next to each other.
template <typename F, typename A, int ORDER, int DIR, int SIGN, int PH, bool GLDS, int NW = 12>
__global__ __launch_bounds__(64 * NW) void tile_displaced_contract_kernel(TileArgs<F, A> a) {
  extern __shared__ __align__(16) unsigned char smem[];
  Cplx<F> *tileBase = reinterpret_cast<Cplx<F> *>(smem);  // 2 (3: GLDS) x [NP][12][32] (buffered over the eigenvectors)
  const size_t tileElems = (size_t)(2 * PH) * 12 * kTileCols;  // padded to 2*PH positions: commits are unconditional
  const int lane = threadIdx.x & 63;
  const int col = lane & 31, half = lane >> 5;
  const int wave = GLDS ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (int)(threadIdx.x >> 6);
  // element index of (position pp, component, line) inside a tile buffer, and the distance between components
  constexpr int kCompStride = GLDS ? 2 * kTileCols : kTileCols;
  auto tileIdx = [&](int pp, int comp, int c) {
    return GLDS ? (((pp >> 1) * 12 + comp) * 2 + (pp & 1)) * kTileCols + c : (pp * 12 + comp) * kTileCols + c;
  };
  const bool computes = wave < kTileTJ * a.nslot;
  const int NP = (DIR >= 1) ? kTileTJ + a.kmax : kTileTJ;

  // ---- which sites this lane works on, and where every staged position lives
  //  DIR >= 1 ("column" tile): 32 lines along mu x TJ consecutive positions j0..j0+TJ-1 (csrc/vector_tile.h).
  //  DIR == 0 ("row" tile): the lines run along x, i.e. along the coalescing direction, so the tile is 2 row groups
  //            x 2 parities of whole x-rows (32 checkerboard entries each): position pp = parity | rowgroup << 1; a
  //            shifted site is another entry of the same row in the other (k odd) or same (k even) parity -- every
  //            eigenvector is read exactly once (1 unit).
  const int wpos = wave % kTileTJ;  // this wave's own position index (jj for the column tile)
  const int slot = wave / kTileTJ;
  const int k = a.k[slot];
  const int blk = xcd_contiguous_block(a.blockOrder);
  int jt = 0, cc = blk, j0 = 0;
  ColumnLine ln = {0, 0, 0, true};           // column tile
  int ePR = 1, rowsPerGroup = 1;             // row tile
  if constexpr (DIR >= 1) {
    if (a.blockOrder & 1) {  // consecutive workgroups = consecutive column groups (adjacent 512-byte runs)
      const int nCC = gridDim.x / a.jtCount;
      jt = a.jtBegin + blk / nCC;
      cc = blk % nCC;
    } else {
      jt = a.jtBegin + blk % a.jtCount;
      cc = blk / a.jtCount;
    }
    j0 = jt * kTileTJ;
    ln = column_line<DIR>(a, cc * kTileCols + col);
  } else {
    ePR = a.X[0] >> 1;                  // checkerboard entries per x-row
    rowsPerGroup = kTileCols / ePR;
    ln.active = col < rowsPerGroup * ePR;  // the host guarantees an even number of whole row groups
  }
  const bool active = ln.active;
  const Cplx<F> *ghostBase = reinterpret_cast<const Cplx<F> *>(a.ghost);
  // x_cb of (row-tile position pp, this lane's column)
  const int colClamped = active ? col : 0;
  auto rowTileXcb = [&](int pp) { return ((2 * cc + (pp >> 1)) * rowsPerGroup) * ePR + colClamped; };

  // source of every position this lane stages (fixed for the whole kernel): plane `wave`, column `col`, positions pp = 2*i + half
  int soff[PH];
  unsigned sghost = 0;
#pragma unroll
  for (int i = 0; i < PH; i++) {
    const int pp = (2 * i + half < NP) ? 2 * i + half : NP - 1;  // surplus slots re-read the last position
    if constexpr (DIR >= 1) {
      soff[i] = column_stage_offset<ORDER, DIR, SIGN>(a, ln, j0, pp, wave, 1u << i, sghost);
    } else {
      soff[i] = (int)((int64_t)(pp & 1) * a.parity_offset + comp_offset<ORDER>(wave, a.stride, rowTileXcb(pp)));
    }
  }

  // ---- my site, and the LDS slots of my v(x) and of my shifted v(x +- k mu)
  TileItem it;
  int colS = col;
  if constexpr (DIR >= 1) {
    it = column_item<SIGN>(a, ln, j0, wpos, k);
  } else {
    it.ppL = wpos;
    it.pmine = wpos & 1;
    it.xmine = rowTileXcb(wpos);
    int c[4];
    get_coords(c, it.xmine, a.X, it.pmine);
    int xs = c[0] + ((SIGN == MUGIQ_HIP_DISP_SIGN_PLUS) ? k : -k);
    xs %= a.X[0];
    if (xs < 0) xs += a.X[0];
    it.ppS = (wpos ^ (k & 1));                   // parity flips for odd k, same row group
    colS = (col / ePR) * ePR + (xs >> 1);        // same row, entry x0' / 2
  }

  Cplx<A> Wr[9];
  const bool unitW = a.E[slot] == nullptr;
  if (!unitW) {
    load_path_link<F, A>(Wr, a.E[slot], it.pmine, it.xmine, a.volumeCB);
  } else {  // the ultra-local loop carried as a slot: k = 0, W = 1
#pragma unroll
    for (int i = 0; i < 9; i++) Wr[i] = Cplx<A>{A(i % 4 == 0 ? 1 : 0), A(0)};
  }
  Cplx<A> acc[8];  // acc[be*2 + a2], al = 2*half + a2
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i] = Cplx<A>{A(0), A(0)};

  // this wave's arithmetic on a tile buffer; where it commits staging slot i (plane `wave`, positions 2*i + half); transfer i of wave w
  // is plane w of the position pair i (its lane halves carry positions 2 i | 2 i + 1), waves 12-15 of the 16-wave form only compute
#define MUGIQ_TILE_COMPUTE(tile_, s_)                                                                                  \
  {                                                                                                                    \
    const Cplx<F> *tile = tile_;                                                                                       \
    const A s = s_;                                                                                                    \
    if (computes) MUGIQ_VT_COMPUTE(kCompStride, tile + tileIdx(it.ppL, 0, col), tile + tileIdx(it.ppS, half * 6, colS), s, unitW)       \
  }
#define MUGIQ_TILE_COMMIT_AT(i) ((2 * i + half) * 12 + wave) * kTileCols + col
  if constexpr (GLDS) {
    MUGIQ_VT_PIPELINE_GLDS(PH, NW == 12 || wave < 12, (size_t)wave * 2 * kTileCols, 24 * kTileCols, MUGIQ_TILE_COMPUTE)
  } else {
    MUGIQ_VT_PIPELINE_REGISTERS(PH, MUGIQ_TILE_COMMIT_AT, MUGIQ_TILE_COMPUTE)
  }
#undef MUGIQ_TILE_COMMIT_AT
#undef MUGIQ_TILE_COMPUTE
  // ---- epilogue: the two lane halves of a wave hold the same 32 sites
  if (computes) {
    MUGIQ_VT_EXCHANGE_HALVES(32)
    if (active) MUGIQ_VT_STORE_TRACES(a.out[slot], it.xmine + it.pmine * a.volumeCB)
  }
}

// g: tile32_launch_geometry of this launch (csrc/fused_form.cpp)
template <typename F, typename A, int ORDER> static int launch_tile(TileArgs<F, A> a, int dir, int sign, const Tile32Launch &g, hipStream_t stream) {
  unsigned nblocks = ((a.numCols + kTileCols - 1) / kTileCols) * a.jtCount;
  if (dir == 0) {  // row tile: 2 groups of kTileCols/(X0/2) whole x-rows per workgroup
    const int ePR = a.X[0] / 2, rpg = kTileCols / ePR;
    nblocks = (unsigned)(a.volumeCB / ePR / rpg / 2);
  }
  // workgroup order, measured on MI355X (48.48.24.24, 100 eigenvectors): XCD-contiguous with the tiles along mu as the
  // fastest index is 2.5 % (fp64) / 1.5 % (fp32) faster than the plain order
  a.blockOrder = g.block_order(nblocks);
  return dispatch_dir_sign(dir, sign, [&](auto D, auto S) -> int {
    constexpr int DIR = decltype(D)::value, SIGN = decltype(S)::value;
    auto launch = [&](auto kern) { return launch_vector_tile(kern, nblocks, g.waves, g.ldsBytes, stream, a); };
    if constexpr (std::is_same<F, double>::value && ORDER == 2 && DIR >= 1) {
      if (g.glds)  // (tile_entry adds the fourth slot only where glds holds)
        return g.waves == 16 ? launch(tile_displaced_contract_kernel<F, A, ORDER, DIR, SIGN, 4, true, 16>)
                             : launch(tile_displaced_contract_kernel<F, A, ORDER, DIR, SIGN, 4, true, 12>);
    }
    if (g.ph == 4) return launch(tile_displaced_contract_kernel<F, A, ORDER, DIR, SIGN, 4, false, 12>);
    // 8 positions per lane: column tiles over fp32 storage.  A row tile stages its kTileTJ positions, never more, and two fp64 buffers of
    // 16 padded positions are 192 KB, which no admission passes (tile32_admits): there are no such instances
    static_assert(2 * (size_t)16 * kTileMaxPos * 12 * kTileCols > kFusedMaxLds, "two fp64 buffers of kTileMaxPos positions fit: build the fp64 PH = 8 instances");
    if constexpr (DIR >= 1 && sizeof(F) == 4) return launch(tile_displaced_contract_kernel<F, A, ORDER, DIR, SIGN, kTileMaxPos / 2, false, 12>);
    return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "vector tile: no instance stages %d positions per lane along direction %d over %d-byte storage (internal)",
                     g.ph, DIR, (int)sizeof(F));
  });
}

// ultra_d != NULL: also produce the ultra-local loop (k = 0, W = 1) into ultra_d, as a fourth slot of the 16-wave form; *carried
// says whether that was possible (fp64 FLOAT2 column tiles staged global -> LDS, at most three displaced slots)
template <typename F, typename A, int ORDER>
int tile_entry(const FusedForm &form, void *loop_d, const MugiqHipSpinorField *ev, const double *sigma, int nVec, const void *const *E_d,
               const int *kvals, int nK, int sign, const void *ghost_d, int layers, int region, hipStream_t stream, void *ultra_d, int *carried) {
  const int dir = form.dir;
  TileArgs<F, A> a;
  int st = fill_vector_tile_args(a, form, ev, sigma, nVec, ghost_d, layers, region, stream);
  if (st) return st;
  const int64_t slot_stride = (int64_t)16 * 2 * ev[0].volumeCB;
  if (carried) *carried = 0;
  const int nJT = dir == 0 ? 1 : ev[0].X[dir] / kTileTJ;  // (the row tile is not cut along x: one "tile", or X0 = 2 would launch nothing)
  // the ultra-local slot is produced for the WHOLE lattice or not at all: a launch restricted to the interior or the boundary
  // tiles would write only part of it (and none of it where that region is empty), so it is taken along with REGION_ALL only
  if (region != MUGIQ_HIP_REGION_ALL) ultra_d = nullptr;
  for (int k0 = 0; k0 < nK; k0 += kTileMaxSlots) {
    fill_vector_tile_slots(a, E_d, kvals, k0, std::min(nK - k0, kTileMaxSlots));
    for (int s = 0; s < kTileCarry; s++) a.out[s] = static_cast<Cplx<A> *>(loop_d) + (int64_t)(k0 + (s < a.nslot ? s : 0)) * slot_stride;
    bool withUltra = false;
    // room for it: a free slot of the 12-wave forms, or the fourth slot of the 16-wave form (global -> LDS staging only)
    if (ultra_d && k0 == 0 && nK <= kTileMaxSlots && (nK < kTileMaxSlots || tile32_launch_geometry(form, nK, a.kmax).glds)) {
      a.E[a.nslot] = nullptr;
      a.k[a.nslot] = 0;
      a.out[a.nslot] = static_cast<Cplx<A> *>(ultra_d);
      a.nslot++;
      withUltra = true;
    }
    tile_range(region, form.partitioned, sign, nJT, a.kmax, kTileTJ, a.jtBegin, a.jtCount);
    if (a.jtCount > 0) {
      st = launch_tile<F, A, ORDER>(a, dir, sign, tile32_launch_geometry(form, a.nslot, a.kmax), stream);
      if (st) return st;
      if (withUltra && carried) *carried = 1;  // only now: a launch that covers the whole lattice did write the slot
    }
  }
  return MUGIQ_HIP_SUCCESS;
}

#define MUGIQ_TILE_INST(F, A, O)                                                                                                 \
  template int tile_entry<F, A, O>(const FusedForm &, void *, const MugiqHipSpinorField *, const double *, int, const void *const *, const int *, \
                                   int, int, const void *, int, int, hipStream_t, void *, int *);
MUGIQ_TILE_INST(double, double, 2)
MUGIQ_TILE_INST(double, double, 4)
MUGIQ_TILE_INST(float, float, 2)
MUGIQ_TILE_INST(float, float, 4)
MUGIQ_TILE_INST(float, double, 2)
MUGIQ_TILE_INST(float, double, 4)
#undef MUGIQ_TILE_INST

}  // namespace mugiq
