// Which kernel an MG transfer call runs on, and with what launch geometry: decided once, on the host, from the transfer descriptor alone.
// Nothing here makes a HIP call or includes device code.  transfer_geom is the one place that derives a level's geometry (the kernels of
// csrc/prolong.hip and csrc/restrict.hip take it in their argument structs), transfer_switches_from_env the only reader of the four
// environment switches of the MG transfers (named there, in csrc/transfer_form.cpp, and nowhere else in csrc/).  The launchers take the
// form they are given and read no size from anywhere else, so what admits a shape is what launches it; the query
// mugiq_hip_transfer_form reports the same forms without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>

#include "mugiq_hip.h"

namespace mugiq {

constexpr size_t kTransferMaxLds = 160 * 1024;  // LDS of one workgroup (gfx950)
constexpr int kTransferMaxNV = 64;              // n_vec of a finest-level transfer (validate_transfer)

// ---- tile constants the forms and the kernels of csrc/prolong.hip share
constexpr int kPrTile = 16;    // vector prolongator: sites per workgroup
constexpr int kPrGroups = 16;  // ... eigenvector groups per workgroup
constexpr int kCmS = 16;       // matrix-pipe kernels: sites per round = columns of one MFMA
constexpr int kPmWaves = 8;    // matrix-pipe prolongator: waves per workgroup (even ones take chirality 0, odd ones chirality 1)
constexpr int kPmPairs = 4;    // ... eight-eigenvector blocks a wave keeps resident (measured: 12-16 blocks per pass beat 24 and 8)

// ---- the geometry of one level: finer lattice X, aggregates bs, coarser lattice Xc = X / bs.  A plain struct: kernel arguments hold it.
struct TransferGeom {
  int X[4], Xc[4], bs[4];
  int aggVol, volumeCB, volumeCBc;
};
TransferGeom transfer_geom(const MugiqHipTransfer &T);
// the fields of the coarser side of a level as the library lays them out itself, without a body: nSpin 2, nColor = n_vec, no pad
MugiqHipCoarseField coarse_side_layout(const MugiqHipTransfer &T);

// ---- the switches.  Read once per public call and passed down by value (never cached: the tests change the environment between calls
// of one process).
struct TransferSwitches {
  bool mgPlan = true;              // false: prolong-contract keeps the per-eigenvector kernel (no coarse-grid plan)
  bool mgMfma = true;              // false: the congruence of the coarse plan stays on the vector kernel
  bool prolongMfma = true;         // false: prolongate-to-fine stays on the vector kernel
  int passBlocks = 4 * kPmPairs;   // matrix-pipe prolongator: blocks of eight eigenvectors per pass at most (experiments: 1 .. 4 kPmPairs)
};
TransferSwitches transfer_switches_from_env();

// ---- prolongate-to-fine (mugiq_hip_prolongate_batched).  Families: MUGIQ_HIP_PROLONG_FAMILY_*
struct ProlongForm {
  int family = 0;
  int precision = 0, order = 0;  // of the fine fields (the transfer's precision)
  int threads = 0, workgroups = 0;  // per launch
  size_t ldsBytes = 0;              // dynamic LDS per workgroup
  int passes = 0, blocksPerPass = 0;  // matrix pipe: launches, and blocks of eight eigenvectors per launch (the last one may take fewer)
  // the head of the per-stream workspace the call may take (the packed coarse vectors of the matrix-pipe form).  The same for every
  // family, so that a caller who keeps data of its own behind it lays its workspace out alike under every switch
  size_t workspaceBytes = 0;
  TransferGeom geom;
};
ProlongForm select_prolong_form(const MugiqHipTransfer &T, int finePrecision, int fineOrder, int nVec, const TransferSwitches &sw);

// ---- prolong-contract (mugiq_hip_prolongate_contract_batched).  Families: MUGIQ_HIP_CONTRACT_FAMILY_*; only what the family uses is set
struct ContractForm {
  int family = 0;
  int precision = 0, loopPrecision = 0;  // storage (the transfer's), accumulation
  int threads = 0, workgroups = 0;  // of the congruence (coarse plan) or of the per-eigenvector kernel (direct)
  size_t ldsBytes = 0;              // dynamic LDS per workgroup of that kernel (coarse_outer_kernel's LDS is static)
  int JC = 0, SPR = 0, NH = 0;      // vector congruence: null vectors per lane chunk, sites per round, chunks (lanes) per (site, chi, chi')
  int outerB = 0;                   // coarse plan: the coarse_outer_kernel instance, (2 n_vec + 15) / 16
  bool glds = false;                // matrix-pipe congruence: the V tile is staged global -> LDS into two buffers
  size_t tableBytes = 0, scratchBytes = 0;  // coarse plan: [pointer table | 1/sigma], and that plus C in the per-stream scratch
  TransferGeom geom;
};
ContractForm select_prolong_contract_form(const MugiqHipTransfer &T, int loopPrecision, int nVec, const TransferSwitches &sw);

// LDS of the kernels, by the functions their launchers instantiate them with
constexpr size_t prolong_tile_lds(int precision, int NV) { return (size_t)2 * precision * 12 * NV * kPrTile; }  // V rows of 16 sites
constexpr size_t congruence_lds(int precision, int loopPrecision, int NV, int SPR) {  // C(X), the SPR x 16 block sums, 4 spins of V rows
  return (size_t)2 * loopPrecision * ((size_t)4 * NV * NV + (size_t)SPR * 16) + (size_t)2 * precision * 4 * NV * SPR;
}
constexpr size_t congruence_mfma_tile_lds(int NV) { return (size_t)16 * 12 * NV * kCmS; }         // the V tile of a round, widened to fp64
constexpr size_t congruence_mfma_red_lds(int NV) { return (size_t)8 * (NV / 2) * kCmS * 8; }      // the partial blocks of the NV / 2 waves
constexpr bool congruence_mfma_glds(int precision, int NV) {
  return precision == 8 && 2 * congruence_mfma_tile_lds(NV) + congruence_mfma_red_lds(NV) <= kTransferMaxLds;
}
// The vector prolongator stages V in LDS where the tile fits, else reads it from global memory.  Only an fp64 tile (n_vec > 53) can fail
// to fit, so the kernel without staging exists for fp64 storage only
static_assert(prolong_tile_lds(4, kTransferMaxNV) <= kTransferMaxLds, "an fp32 V tile always fits the LDS of a workgroup");

}  // namespace mugiq
