// select_fused_form: the one place that decides which kernel a fused displaced entry runs on (see csrc/fused_form.h).  Host only.
#include "fused_form.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace mugiq {

int set_error(int status, const char *fmt, ...);  // host_api.cpp

static int env_int(const char *name, int unset) {
  const char *e = getenv(name);
  return e ? atoi(e) : unset;
}

FusedSwitches fused_switches_from_env() {
  FusedSwitches s;
  s.fusedTile = env_int("MUGIQ_HIP_FUSED_TILE", 1);
  if (const char *e = getenv("MUGIQ_HIP_FUSED_TUNE")) sscanf(e, "%d,%d,%d", &s.tuneNt, &s.tuneSwizzle, &s.tuneRemap);
  s.tileMfma = env_int("MUGIQ_HIP_TILE_MFMA", 1) != 0;
  s.tileCols = env_int("MUGIQ_HIP_TILE_COLS", 0);
  s.tileGlds = env_int("MUGIQ_HIP_TILE_GLDS", 1) != 0;
  s.tileOrder = env_int("MUGIQ_HIP_TILE_ORDER", 2);
  s.tile16Tj = env_int("MUGIQ_HIP_TILE16_TJ", 4) == 8 ? 8 : 4;
  s.tile16Glds = env_int("MUGIQ_HIP_TILE16_GLDS", 1) != 0;
  s.mfmaTj = env_int("MUGIQ_HIP_MFMA_TJ", 0);
  s.mfmaRow = env_int("MUGIQ_HIP_MFMA_ROW", 1) != 0;
  s.mfmaRowWaves = env_int("MUGIQ_HIP_MFMA_ROW_WAVES", 0);
  s.mfmaStorage = env_int("MUGIQ_HIP_MFMA_STORAGE", 1) != 0;
  s.packInEntry = env_int("MUGIQ_HIP_PACK_IN_ENTRY", 1) != 0;
  s.gaugeFromLinks = env_int("MUGIQ_HIP_GAUGE_FROM_LINKS", 1) != 0;
  return s;
}

// ---- the matrix-pipe tile ------------------------------------------------------------------------------------------------------
// The column tile: the first TJ of {8, 12, 4} that divides the extent and keeps TJ + Kmax within the staged positions of its line
// count (MUGIQ_HIP_MFMA_TJ fixes it); 0 = none.  (two-sided: 8 or 4 only -- a 12-position left image next to the right one exceeds
// the LDS of a workgroup; storage types other than fp64 FLOAT2 come with the 16-line tiles only)
static int mfma_tile_tj(const FusedForm &f, int kmax, int nSlots, bool partitioned) {
  // 12 x 16 sites (1 + K/12 units staged per site) where it keeps its registers -- three groups per wave: up to three slots -- and the
  // line is not partitioned (of 24 / 12 = 2 tiles along the line one would be a boundary tile): "+z:1,3;+t:1,3" N_ev 200 32.6 against
  // 33.4 ms.  Else 8 x 16, then 12 x 16 (spills with four slots), then 4 x 32 (512-byte runs, but 1 + K/4 units).
  const int first = (!partitioned && nSlots < kMT_MaxSlots) ? 12 : 8;
  for (int tj : {first, 8, 12, 4}) {
    if (f.sw.mfmaTj && tj != f.sw.mfmaTj) continue;
    if ((f.reduced() && tj == 4) || (f.two && tj == 12)) continue;
    if (f.X[f.dir] % tj != 0 || tj + kmax > (tj == 4 ? 8 : 16)) continue;
    return tj;
  }
  return 0;
}

// mu = x: R whole rows per workgroup of W waves, G = 2 | 3 groups of 4 sites per wave: R X0 = 16 G W sites.  Two workgroups of 8
// waves per CU where the rows allow, else one of 16 (MUGIQ_HIP_MFMA_ROW_WAVES fixes it).
static bool mfma_row_geometry(const FusedForm &f, MfmaLaunch &g) {
  const int epr = f.X[0] / 2, nRows = f.volumeCB / epr;
  if (epr % 4 != 0) return false;
  for (int w : {8, 16}) {  // (X0 = 48, N_ev 200, spill-free kernels: two workgroups of 8 waves per CU 13.1 ms per entry, one of 16 13.6)
    if (f.sw.mfmaRowWaves && w != f.sw.mfmaRowWaves) continue;
    if ((f.reduced() || f.two) && w != 8) continue;  // (... and with the 8-wave row tile only; so are the two-sided tiles)
    for (int grp : {3, 2}) {
      if (f.two && f.reduced() && grp != 2) continue;  // (two-sided, storage other than fp64 FLOAT2: 3 groups per wave spill)
      if ((2 * grp * w) % epr != 0) continue;
      const int r = 2 * grp * w / epr;
      if (nRows % r != 0 || r * 8 * (epr + kMT_MaxLength / 2) > 64 * w) continue;
      // > R (X0/2 + 4) (the entry behind the rows holds the zero of the padded operand lanes), and 4 mod 16 entries: 16 banks of
      // phase per component
      const int chunk = (r * (epr + kMT_MaxLength / 2) + 12) / 16 * 16 + 4;
      if (24 * chunk > (w == 8 ? kMT_BufElems / 2 : kMT_BufElems)) continue;  // the LDS image of a tile buffer
      g.rowGroups = grp, g.rows = r, g.waves = w, g.rowChunk = chunk;
      return true;
    }
  }
  return false;
}

MfmaLaunch mfma_launch_geometry(const FusedForm &f, int nSlots, int kmax) {
  MfmaLaunch g;
  g.orderBits = f.sw.tileOrder & 2;
  g.rowOrderOff = f.dir == 0;
  size_t bufElems = kMT_BufElems, products;
  if (f.dir == 0) {
    if (!mfma_row_geometry(f, g)) return g;
    g.tj = f.X[0];  // one "tile" along mu
    g.lines = 16 * g.rowGroups;
    g.staged = f.X[0] + kMT_MaxLength;
    g.leftBufElems = f.two ? 24 * g.rowChunk : 0;  // (the left image has the layout of the right one)
    if (g.waves == 8) bufElems = kMT_BufElems / 2;
    products = (size_t)4 * g.rowGroups * g.waves;
  } else {
    // the tile of THIS launch (its slots and the positions it stages), else the entry's
    g.tj = mfma_tile_tj(f, kmax, nSlots, f.partitioned != 0);
    if (!g.tj) g.tj = mfma_tile_tj(f, f.kmax, kMT_MaxSlots, true);
    if (!g.tj) return g;
    g.lines = g.tj == 4 ? 32 : 16;
    g.waves = kMT_Waves;
    g.staged = g.tj + kmax;
    g.leftBufElems = f.two ? mt_left_buf_elems(g.tj) : 0;
    products = (size_t)g.tj * g.lines;
  }
  g.ldsBytes = std::max(2 * bufElems + 2 * (size_t)g.leftBufElems, 16 * products) * 16;  // complex double
  g.ok = g.ldsBytes <= kMT_MaxLds;
  return g;
}

// fp64 / fp32 storage in either order, ascending lengths up to 8 (from 1 without a gap where the tile has to build the gauge itself,
// from W_1 .. W_Kmax = the links it is handed; any ascending list where the caller has built it)
static bool mfma_admits(const FusedForm &f, int64_t elems, const int *kvals, int nK, bool gaugeGiven) {
  const FusedSwitches &sw = f.sw;
  if (!sw.tileMfma || sw.fusedTile == 0 || sw.tileCols != 0 || !sw.tileGlds) return false;  // (the vetoes: see FusedSwitches)
  if ((f.precision != 8 && f.precision != 4) || (f.order != 2 && f.order != 4)) return false;
  if (!sw.mfmaStorage && f.reduced()) return false;
  if (elems >= (1LL << 31)) return false;  // the kernel keeps 32-bit element offsets
  for (int i = 0; i < nK; i++)
    if (kvals[i] < 1 || (i > 0 && kvals[i] <= kvals[i - 1]) || (!gaugeGiven && kvals[i] != i + 1)) return false;
  if (f.kmax > kMT_MaxLength || f.kmax > f.X[f.dir]) return false;
  // whole x rows: no ghost handling, and the row tile keeps 32-bit BYTE offsets
  if (f.dir == 0 && (!sw.mfmaRow || elems >= (1LL << 28) || f.partitioned)) return false;
  return mfma_launch_geometry(f, kMT_MaxSlots, f.kmax).ok;
}

// ---- the 32-line vector tile ---------------------------------------------------------------------------------------------------
Tile32Launch tile32_launch_geometry(const FusedForm &f, int nSlots, int kmax) {
  Tile32Launch g;
  g.staged = f.dir >= 1 ? kTileTJ + kmax : kTileTJ;
  g.ph = g.staged <= 8 ? 4 : kTileMaxPos / 2;
  // global -> LDS staging with three buffers: fp64 FLOAT2 column tiles of at most 8 positions
  g.glds = !f.reduced() && f.dir >= 1 && kTileTJ + kmax <= 8 && f.sw.tileGlds;
  g.bufferBytes = (size_t)2 * f.precision * (2 * g.ph) * 12 * kTileCols;  // padded positions
  g.ldsBytes = (g.glds ? 3 : 2) * g.bufferBytes;
  g.waves = nSlots == kTileCarry ? 16 : 12;
  g.orderBits = f.sw.tileOrder & 3;
  return g;
}

static bool tile32_admits(const FusedForm &f) {
  if (f.sw.fusedTile == 0 || (f.sw.fusedTile == 2 && f.dir == 0)) return false;
  if (f.dir == 0) {  // row tile: whole x-rows in LDS, no ghost handling
    const int ePR = f.X[0] / 2;
    if (f.partitioned || ePR > kTileCols || f.kmax >= f.X[0]) return false;
    if ((f.volumeCB / ePR) % (2 * (kTileCols / ePR)) != 0) return false;
  } else {
    if (f.X[f.dir] % kTileTJ != 0 || f.kmax > f.X[f.dir]) return false;  // the staged window wraps at most once around the lattice
    if (kTileTJ + f.kmax > kTileMaxPos) return false;
  }
  // (the bound is that of two buffers even where the launch takes three: those are the 4-position-pair tiles, which fit)
  return 2 * tile32_launch_geometry(f, kTileMaxSlots, f.kmax).bufferBytes <= kFusedMaxLds;
}

// ---- the 16-line vector tile ---------------------------------------------------------------------------------------------------
static int gcd_int(int x, int y) { return y == 0 ? x : gcd_int(y, x % y); }

Tile16Launch tile16_launch_geometry(const FusedForm &f, int nSlots, int kmax) {
  Tile16Launch g;
  int minWaves;
  if (f.dir == 0) {  // row tile: whole x rows in LDS, no ghost handling
    const int ePR = f.X[0] / 2;
    if (f.partitioned || kmax >= f.X[0]) return g;
    g.m = ePR / gcd_int(kT16Cols, ePR);  // lcm(16, ePR) / 16
    g.npc = g.np = 2 * g.m;
    if (g.npc > kT16MaxItems || f.volumeCB % (g.m * kT16Cols) != 0) return g;
    g.maxSlots = std::min(kT16MaxSlots, kT16MaxItems / g.npc);
    minWaves = 2;
  } else {
    g.tj = f.sw.tile16Tj;
    if (f.X[f.dir] % g.tj != 0 || kmax > f.X[f.dir] || g.tj + kmax > kT16MaxPos) return g;
    g.npc = g.tj;
    g.np = g.tj + kmax;
    g.maxSlots = kT16MaxSlots;
    minWaves = 6 * g.tj / 4;  // idle waves of a launch with fewer slots still stage
  }
  g.ok = true;
  g.staged = g.np;
  g.waves = std::max(minWaves, (g.npc * nSlots + 1) / 2);  // two items per wave
  const int nthreads = 64 * g.waves;
  g.phl = (g.np * kT16Row + nthreads - 1) / nthreads;
  g.phlSel = g.phl <= 2 ? 2 : (g.phl <= 4 ? 4 : 8);
  g.bufferBytes = (size_t)2 * f.precision * g.phlSel * nthreads;
  // global -> LDS staging with three buffers where they fit: fp64 FLOAT2 storage
  g.glds = !f.reduced() && 3 * g.bufferBytes <= kFusedMaxLds && f.sw.tile16Glds;
  g.ldsBytes = (g.glds ? 3 : 2) * g.bufferBytes;
  g.orderBits = f.sw.tileOrder & 2;
  return g;
}

// Measured (48.48.24.24 fp64, 100 eigenvectors, three slots): row tile 9.3 ms here against 11.3 ms with 32-line positions
// (24 of 32 lanes busy at X0 = 48); column tiles 10.6-10.9 ms here against 8.9 ms (256-byte instead of 512-byte runs per
// load instruction; the two workgroups per CU did not buy the overlap hoped for).  So by default the 16-line kernel takes the ROW
// tiles whose rows do not fill 32-line positions (32 % (X0/2) != 0) and whatever the 32-line one cannot take;
// MUGIQ_HIP_TILE_COLS = 16 | 32 forces one generation for everything it can take.
static bool tile16_admits(const FusedForm &f, bool tile32Applies) {
  if (f.sw.tileCols == 32) return false;
  if (f.sw.tileCols != 16 && tile32Applies && !(f.dir == 0 && 32 % (f.X[0] / 2) != 0)) return false;
  if (f.sw.fusedTile == 0 || (f.sw.fusedTile == 2 && f.dir == 0)) return false;
  // staging loads per lane with the fewest threads a launch may have (one slot); two staging tiles (three when they fit)
  const Tile16Launch g = tile16_launch_geometry(f, 1, f.kmax);
  return g.ok && g.phl <= 8 && 2 * g.bufferBytes <= kFusedMaxLds;
}

FusedForm select_fused_form(const MugiqHipSpinorField &ev, int dir, const int *kvals, int nK, int partitioned, bool gaugeGiven, bool two,
                            int loopPrecision, const FusedSwitches &sw, bool allowMatrixPipe) {
  FusedForm f;
  for (int d = 0; d < 4; d++) f.X[d] = ev.X[d];
  f.volumeCB = ev.volumeCB, f.precision = ev.precision, f.order = ev.field_order, f.loopPrecision = loopPrecision;
  f.dir = dir, f.partitioned = partitioned, f.two = two, f.sw = sw;
  for (int i = 0; i < nK; i++) f.kmax = std::max(f.kmax, kvals[i]);
  const int64_t elems = 2 * (int64_t)ev.parity_offset;
  if (allowMatrixPipe && mfma_admits(f, elems, kvals, nK, gaugeGiven)) {
    f.family = dir == 0 ? MUGIQ_HIP_FUSED_FAMILY_MFMA_ROW : MUGIQ_HIP_FUSED_FAMILY_MFMA_COLUMN;
    f.kernel = dir == 0 ? MUGIQ_HIP_ENTRY_KERNEL_MFMA_ROW : MUGIQ_HIP_ENTRY_KERNEL_MFMA_COLUMN;
    // (the row tile has no four-slot instance: it takes no ultra-local loop along)
    f.slotsPerLaunch = two ? mt_two_max_slots(dir, !f.reduced()) : dir == 0 ? kMT_MaxSlots - 1 : kMT_MaxSlots;
    f.gaugeBytes = axial_gauge_bytes_of(ev, dir, f.kmax);
    // face layers of z / t: fp64 FLOAT2, rows of a workgroup within one (z, t), face entry within its slice in 20 bits of the kernel
    if (dir == 0 && !two && sw.packInEntry && !f.reduced() && ev.X[1] % mfma_launch_geometry(f, 1, f.kmax).rows == 0 &&
        (int64_t)ev.X[1] * (ev.X[0] / 2) < (1 << 20))
      f.packCapacity = kMT_MaxPack;
    return f;
  }
  if (two) return f;  // (no two-sided form of the vector tiles or of the streaming kernel)
  const bool offsets32 = elems < (1LL << 31);  // the tile kernels keep 32-bit element offsets
  const bool tile32 = offsets32 && tile32_admits(f);
  if (offsets32 && tile16_admits(f, tile32)) {
    f.family = MUGIQ_HIP_FUSED_FAMILY_TILE16;
    f.slotsPerLaunch = tile16_launch_geometry(f, 1, f.kmax).maxSlots;
  } else if (tile32) {
    f.family = MUGIQ_HIP_FUSED_FAMILY_TILE32;
    f.slotsPerLaunch = kTileMaxSlots;
  } else {
    f.family = MUGIQ_HIP_FUSED_FAMILY_STREAMING;
    f.slotsPerLaunch = kFusedMaxSlots;
  }
  f.kernel = f.family == MUGIQ_HIP_FUSED_FAMILY_STREAMING ? MUGIQ_HIP_ENTRY_KERNEL_STREAMING : MUGIQ_HIP_ENTRY_KERNEL_VECTOR_TILE;
  return f;
}

bool axial_gauge_from_links_possible(const MugiqHipSpinorField &ev, const MugiqHipGaugeField &U, int kmax, int dir, int sign,
                                     const FusedSwitches &sw) {
  if (U.precision != ev.precision || !sw.gaugeFromLinks) return false;
  const int R = U.R[dir];
  return R == 0 || (sign == MUGIQ_HIP_DISP_SIGN_PLUS ? kmax <= R + 1 : kmax <= R);
}

}  // namespace mugiq

extern "C" int mugiq_hip_fused_form(const MugiqHipSpinorField *ev, int twoSided, int dispDir, const int *kValues, int nK, int partitioned,
                                    int gaugeGiven, int loopPrecision, MugiqHipFusedForm *out) {
  using namespace mugiq;
  const char *who = "mugiq_hip_fused_form";
  if (!ev || !kValues || !out || nK < 1 || dispDir < 0 || dispDir > 3)
    return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: NULL argument, nK = %d < 1 or direction %d", who, nK, dispDir);
  for (int d = 0; d < 4; d++)
    if (ev->X[d] < 2 || ev->X[d] % 2 || ev->volumeCB <= 0) return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: ev carries no geometry", who);
  const FusedForm f = select_fused_form(*ev, dispDir, kValues, nK, partitioned != 0, gaugeGiven != 0, twoSided != 0,
                                        loopPrecision ? loopPrecision : ev->precision, fused_switches_from_env(), true);
  memset(out, 0, sizeof(*out));
  out->kernel = f.kernel, out->family = f.family, out->slotsPerLaunch = f.slotsPerLaunch, out->packCapacity = f.packCapacity;
  out->gaugeBytes = (long long)f.gaugeBytes;
  if (f.family == MUGIQ_HIP_FUSED_FAMILY_NONE) return MUGIQ_HIP_SUCCESS;
  // the first launch: its slots (no ultra-local loop riding along) and its longest length
  const bool mfma = fused_form_is_mfma(f);
  out->nSlots = mfma ? fused_even_slots(nK, f.slotsPerLaunch) : std::min(nK, f.slotsPerLaunch);
  for (int i = 0; i < out->nSlots; i++) out->kmax = std::max(out->kmax, kValues[i]);
  FusedLaunchBase b;
  if (mfma) {
    const MfmaLaunch g = mfma_launch_geometry(f, out->nSlots, out->kmax);
    out->tj = g.tj, out->lines = g.lines, out->rowGroups = g.rowGroups, out->rows = g.rows, out->rowChunk = g.rowChunk;
    out->leftBufElems = g.leftBufElems;
    b = g;
  } else if (f.family == MUGIQ_HIP_FUSED_FAMILY_TILE32) {
    const Tile32Launch g = tile32_launch_geometry(f, out->nSlots, out->kmax);
    out->tj = kTileTJ, out->lines = kTileCols, out->ph = g.ph, out->glds = g.glds;
    b = g;
  } else if (f.family == MUGIQ_HIP_FUSED_FAMILY_TILE16) {
    const Tile16Launch g = tile16_launch_geometry(f, out->nSlots, out->kmax);
    out->tj = g.tj, out->lines = kT16Cols, out->npc = g.npc, out->np = g.np, out->m = g.m, out->phl = g.phlSel, out->glds = g.glds;
    b = g;
  } else {
    b.waves = out->nSlots;  // one wave per slot over 64 sites
  }
  out->waves = b.waves, out->staged = b.staged, out->ldsBytes = (long long)b.ldsBytes;
  return MUGIQ_HIP_SUCCESS;
}
