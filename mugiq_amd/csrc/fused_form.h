// Which kernel a fused displaced entry runs on, and with what launch geometry: decided once, on the host, from descriptors alone.
// select_fused_form and the *_launch_geometry functions make no HIP call and include no device code; fused_switches_from_env is the
// only reader of the MUGIQ_HIP_* switches of the fused kernels (csrc/fused.hip, fused_tile.hip, fused_tile16.hip, fused_mfma*.hip).
// The admission checks of select_fused_form call the launch-geometry function the launch itself calls, so the two cannot disagree;
// fused_entry, make_loop_plan and the query mugiq_hip_fused_form all go through it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "mugiq_hip.h"

namespace mugiq {

constexpr size_t kFusedMaxLds = 160 * 1024;  // LDS of one workgroup (gfx950)

// ---- the streaming kernel (csrc/fused.hip)
constexpr int kFusedMaxSlots = 4;

// ---- the 32-line vector tile (csrc/fused_tile.hip)
constexpr int kTileTJ = 4;        // positions along mu per workgroup
constexpr int kTileMaxSlots = 3;  // displaced slots per launch: waves = kTileTJ * nslot <= 12
constexpr int kTileCarry = kTileMaxSlots + 1;  // + the ultra-local loop riding along as a slot with k = 0 (16 waves; GLDS form only)
constexpr int kTileMaxPos = 16;   // TJ + Kmax upper bound
constexpr int kTileCols = 32;     // lines per workgroup (each line is held by two lanes: one per spin half)

// ---- the 16-line vector tile (csrc/fused_tile16.hip)
constexpr int kT16Cols = 16;       // lines per item (each line is held by two lanes: one per spin half)
constexpr int kT16MaxSlots = 3;
constexpr int kT16MaxItems = 24;   // 12 waves
constexpr int kT16MaxPos = 16;     // staged positions: TJ + Kmax upper bound
constexpr int kT16Row = 12 * kT16Cols;  // elements of one staged position

// ---- the matrix-pipe tile (csrc/fused_mfma_kernel.h).  Tile geometries (TJ positions along mu x LN lines per workgroup; 16 waves):
//   TJ =  4, LN = 32: 128 sites, 4 + Kmax <=  8 staged positions, 1 + Kmax/4  units requested per site (the tile of csrc/fused_tile.hip)
//   TJ =  8, LN = 16: 128 sites, 8 + Kmax <= 16 staged positions, 1 + Kmax/8
//   TJ = 12, LN = 16: 192 sites, 12 + Kmax <= 16 staged positions, 1 + Kmax/12
// 4-site groups: TJ LN / 4, an equal share per wave (2 | 2 | 3), group -> (position, 4 consecutive lines).
constexpr int kMT_Waves = 16;
constexpr int kMT_MaxSlots = 4;   // 3 displaced slots + the ultra-local loop riding along (k = 0) per launch
constexpr int kMT_MaxLength = 8;  // lengths 1 .. 8 per entry (launches of three lengths; 4 x 32 tiles: 1 .. 4)
constexpr int kMT_MaxPack = 4;   // face-layer targets a row-tile launch can fill on the way (z and t, low and high side)
constexpr int kMT_Chunk = 68;     // complex elements per chunk: 64 + 4 of bank phase
constexpr int kMT_Chunks = 4 * 12;  // chunks of a tile buffer: 64 / LN positions each, 12 components, <= 4 * 64 / LN staged positions
constexpr int kMT_BufElems = kMT_Chunks * kMT_Chunk;
constexpr size_t kMT_MaxLds = kFusedMaxLds;
// two-sided column tiles: one buffer of the left image holds the TJ own positions (TJ / (64 / LN) position chunks of 12 components)
constexpr int mt_left_buf_elems(int tj) { return tj / (64 / (tj == 4 ? 32 : 16)) * 12 * kMT_Chunk; }
// slots per two-sided launch that compile without scratch (128 VGPRs): 3 on the fp64 FLOAT2 column tiles, else 2
constexpr int mt_two_max_slots(int dir, bool full) { return dir != 0 && full ? 3 : 2; }

// ---- the switches.  Read once per public fused call and once per make_loop_plan, then passed down by value (never cached: the tests
// change the environment between calls of one process).  How they interact:
//   * FUSED_TILE = 0 leaves the streaming kernel only; FUSED_TILE = 2 keeps the vector ROW tiles (mu = x) out -- but not the
//     matrix-pipe row tile, which only looks at FUSED_TILE = 0.
//   * The matrix-pipe tile is also vetoed by TILE_MFMA = 0, by TILE_COLS != 0 (a vector-tile generation was asked for by name) and by
//     TILE_GLDS = 0 (the register-staged vector tile was asked for).
//   * TILE_ORDER: the 32-line tile takes bits 0 and 1 (& 3), the 16-line and the matrix-pipe tiles bit 1 only (& 2).
struct FusedSwitches {
  int fusedTile = 1;       // MUGIQ_HIP_FUSED_TILE: 0 = streaming kernel only, 2 = no vector row tile
  int tuneNt = 1, tuneSwizzle = 1, tuneRemap = 1;  // MUGIQ_HIP_FUSED_TUNE = "nt,swizzle,remap" (streaming kernel; profiles/r01_fused_tune.txt)
  bool tileMfma = true;    // MUGIQ_HIP_TILE_MFMA = 0: no matrix-pipe tile
  int tileCols = 0;        // MUGIQ_HIP_TILE_COLS = 16 | 32: that vector-tile generation for everything it can take
  bool tileGlds = true;    // MUGIQ_HIP_TILE_GLDS = 0: the 32-line tile stages through registers
  int tileOrder = 2;       // MUGIQ_HIP_TILE_ORDER: workgroup -> tile map (bit 1: XCD-contiguous; bit 0: column groups fastest)
  int tile16Tj = 4;        // MUGIQ_HIP_TILE16_TJ = 4 | 8: positions along mu per 16-line column tile
  bool tile16Glds = true;  // MUGIQ_HIP_TILE16_GLDS = 0: the 16-line tile stages through registers
  int mfmaTj = 0;          // MUGIQ_HIP_MFMA_TJ = 4 | 8 | 12 fixes the column tile
  bool mfmaRow = true;     // MUGIQ_HIP_MFMA_ROW = 0: no matrix-pipe row tile
  int mfmaRowWaves = 0;    // MUGIQ_HIP_MFMA_ROW_WAVES = 8 | 16 fixes the row tile's workgroup
  bool mfmaStorage = true; // MUGIQ_HIP_MFMA_STORAGE = 0: the matrix-pipe tile for fp64 FLOAT2 only
  bool packInEntry = true; // MUGIQ_HIP_PACK_IN_ENTRY = 0: the row tile writes no face layers
  bool gaugeFromLinks = true;  // MUGIQ_HIP_GAUGE_FROM_LINKS = 0: the axial gauge always from path-link fields
};
FusedSwitches fused_switches_from_env();

enum FusedFamily {
  FUSED_FAMILY_NONE = 0,  // two-sided without a tile: the step-by-step sequence
  FUSED_FAMILY_MFMA_COLUMN,
  FUSED_FAMILY_MFMA_ROW,
  FUSED_FAMILY_TILE32,
  FUSED_FAMILY_TILE16,
  FUSED_FAMILY_STREAMING
};

struct FusedForm {
  int kernel = MUGIQ_HIP_ENTRY_KERNEL_STEPWISE;  // what mugiq_hip_loop_get_entry_kernel will report
  int family = FUSED_FAMILY_NONE;
  int slotsPerLaunch = 0;  // displaced slots a launch takes at most
  int packCapacity = 0;    // face-layer targets a mu = x entry can write on its way (0: it cannot)
  size_t gaugeBytes = 0;   // the axial gauge of the entry (0: not a matrix-pipe tile)
  // what the launch-geometry functions need of the entry
  int X[4] = {0, 0, 0, 0}, volumeCB = 0, precision = 0, order = 0, loopPrecision = 0;
  int dir = 0, kmax = 0, partitioned = 0;
  bool two = false;
  FusedSwitches sw;
  bool reduced() const { return !(precision == 8 && order == 2); }  // storage other than fp64 FLOAT2
};

// ev: the geometry of ev[0]; kvals: the lengths of the entry; gaugeGiven: the caller holds the axial gauge (any ascending lengths; else
// 1 .. nK); allowMatrixPipe = false: the unitarity check of the links refused the matrix-pipe tile
FusedForm select_fused_form(const MugiqHipSpinorField &ev, int dir, const int *kvals, int nK, int partitioned, bool gaugeGiven, bool two,
                            int loopPrecision, const FusedSwitches &sw, bool allowMatrixPipe);
inline bool fused_form_is_mfma(const FusedForm &f) { return f.family == FUSED_FAMILY_MFMA_COLUMN || f.family == FUSED_FAMILY_MFMA_ROW; }

// Every tile launch: LDS bytes, threads, staged positions, and the workgroup order as a function of the number of workgroups
struct FusedLaunchBase {
  size_t ldsBytes = 0;
  int waves = 0, staged = 0;
  int orderBits = 0;      // of MUGIQ_HIP_TILE_ORDER, masked for the family
  bool rowOrderOff = false;
  int block_order(unsigned nblocks) const { return rowOrderOff ? 0 : nblocks % 8 != 0 ? orderBits & 1 : orderBits; }
};
// nSlots: the slots of THIS launch (the ultra-local loop riding along included); kmax: its longest length
struct MfmaLaunch : FusedLaunchBase {
  bool ok = false;
  int tj = 0, lines = 0;                    // column tile (row tile: tj = X0, one "tile" along mu)
  int rowGroups = 0, rows = 0, rowChunk = 0;  // row tile: 4-site groups per wave, whole x rows per workgroup, chunk stride of their image
  int leftBufElems = 0;                     // two-sided: complex elements of one buffer of the left image
};
MfmaLaunch mfma_launch_geometry(const FusedForm &f, int nSlots, int kmax);
struct Tile32Launch : FusedLaunchBase {
  int ph = 0;             // bound of the positions staged per lane
  bool glds = false;      // staged global -> LDS (three buffers), else through registers (two)
  size_t bufferBytes = 0;
};
Tile32Launch tile32_launch_geometry(const FusedForm &f, int nSlots, int kmax);
struct Tile16Launch : FusedLaunchBase {
  bool ok = false;
  int tj = 0, npc = 0, np = 0, m = 0;  // computed / staged positions per tile; row tile: 16-entry pieces per parity
  int maxSlots = 0, phl = 0, phlSel = 0;  // staging loads per lane, and the kernel instance that bounds them
  bool glds = false;
  size_t bufferBytes = 0;
};
Tile16Launch tile16_launch_geometry(const FusedForm &f, int nSlots, int kmax);
// slots of the next launch when `slotsLeft` are dealt evenly over launches of at most `room` (1 .. 8 with room 3: 3 + 3 + 2)
inline int fused_even_slots(int slotsLeft, int room) {
  const int launchesLeft = (slotsLeft + room - 1) / room;
  return (slotsLeft + launchesLeft - 1) / launchesLeft;
}

// Can the axial gauge of (dir, sign) with lengths up to kmax be taken from the gauge field?  Always along a direction that is not
// partitioned (border 0: periodic line); along a partitioned one as far as the border of the extended field reaches: the continued
// positions need the links at J .. J + kmax - 2 (sign +) or -1 .. -kmax (sign -).
bool axial_gauge_from_links_possible(const MugiqHipSpinorField &ev, const MugiqHipGaugeField &U, int kmax, int dir, int sign,
                                     const FusedSwitches &sw);
inline size_t axial_gauge_bytes_of(const MugiqHipSpinorField &ev, int dir, int kmax) {
  return (size_t)9 * (ev.X[dir] + kmax) * (size_t)(2 * ev.volumeCB / ev.X[dir]) * 16;  // [9][J + kmax][lines] complex double
}

// ---- host set-up shared by the entries and the axial-gauge builders
// the lines of direction dir: x_cb distance of one step (mu = x: 1, unused -- a step along x is half a checkerboard entry)
struct LineGeometry {
  int strideMu, H, numCols, faceCB;  // H = volumeCB / (X[dir] * strideMu); numCols = V / X[dir]
  int64_t ghost_vec_stride;          // complex elements of ghost layers per eigenvector = layers * 24 * faceCB
};
inline LineGeometry line_geometry(const MugiqHipSpinorField &ev, int dir, int layers = 0) {
  long long strideMu = 1;
  for (int d = 0; d < dir; d++) strideMu *= ev.X[d];
  strideMu = dir == 0 ? 1 : strideMu / 2;
  LineGeometry g;
  g.strideMu = (int)strideMu;
  g.H = (int)(ev.volumeCB / (ev.X[dir] * strideMu));
  g.numCols = 2 * ev.volumeCB / ev.X[dir];
  g.faceCB = ev.volumeCB / ev.X[dir];
  g.ghost_vec_stride = (int64_t)layers * 24 * g.faceCB;
  return g;
}
// region 0: every tile along mu | 1: tiles whose shifted reads stay inside the local lattice | 2: tiles that read ghost layers
// (kmax decides how many tiles are boundary tiles; a row tile, nJT = 1 and never partitioned, has no boundary part)
inline void tile_range(int region, int partitioned, int sign, int nJT, int kmax, int tj, int &jtBegin, int &jtCount) {
  jtBegin = 0;
  jtCount = nJT;
  if (region == MUGIQ_HIP_REGION_ALL) return;
  const int nb = partitioned ? std::min(nJT, (kmax + tj - 1) / tj) : 0;  // boundary tiles
  if (region == MUGIQ_HIP_REGION_INTERIOR) {
    jtBegin = sign == MUGIQ_HIP_DISP_SIGN_PLUS ? 0 : nb;
    jtCount = nJT - nb;
  } else {
    jtBegin = sign == MUGIQ_HIP_DISP_SIGN_PLUS ? nJT - nb : 0;
    jtCount = nb;
  }
}

}  // namespace mugiq
