// select_prolong_form / select_prolong_contract_form: the one place that decides which kernel an MG transfer call runs on (see
// csrc/transfer_form.h).  Host only.
#include "internal.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mugiq {

TransferGeom transfer_geom(const MugiqHipTransfer &T) {
  TransferGeom g;
  long long vol = 1, volc = 1;
  g.aggVol = 1;
  for (int d = 0; d < 4; d++) {
    g.X[d] = T.X[d];
    g.bs[d] = T.geoBlockSize[d];
    g.Xc[d] = g.bs[d] > 0 ? g.X[d] / g.bs[d] : 0;  // (a block size < 1 is the validators' to report)
    g.aggVol *= g.bs[d];
    vol *= g.X[d];
    volc *= g.Xc[d];
  }
  g.volumeCB = (int)(vol / 2);
  g.volumeCBc = (int)(volc / 2);
  return g;
}

MugiqHipCoarseField coarse_side_layout(const MugiqHipTransfer &T) {
  const TransferGeom g = transfer_geom(T);
  MugiqHipCoarseField f{};
  f.precision = T.precision, f.nSpin = 2, f.nColor = T.nVec;
  for (int d = 0; d < 4; d++) f.X[d] = g.Xc[d];
  f.volumeCB = f.stride = g.volumeCBc;
  f.parity_offset = (int64_t)2 * f.nColor * f.stride;
  return f;
}

// MUGIQ_HIP_MG_PLAN=direct (that string only) switches the coarse-grid plan off; MUGIQ_HIP_MG_MFMA=0 and MUGIQ_HIP_PROLONG_MFMA=0 the
// matrix-pipe congruence and prolongator; MUGIQ_HIP_PROLONG_PASS_BLOCKS = 1 .. 4 kPmPairs sets the blocks per pass (else ignored)
TransferSwitches transfer_switches_from_env() {
  TransferSwitches s;
  if (const char *e = getenv("MUGIQ_HIP_MG_PLAN")) s.mgPlan = strcmp(e, "direct") != 0;
  if (const char *e = getenv("MUGIQ_HIP_MG_MFMA")) s.mgMfma = atoi(e) != 0;
  if (const char *e = getenv("MUGIQ_HIP_PROLONG_MFMA")) s.prolongMfma = atoi(e) != 0;
  if (const char *e = getenv("MUGIQ_HIP_PROLONG_PASS_BLOCKS")) {
    const int c = atoi(e);
    if (c >= 1 && c <= 4 * kPmPairs) s.passBlocks = c;
  }
  return s;
}

// The per-eigenvector vector kernel (prolong_kernel): 16 sites x 16 eigenvector groups per workgroup.  redBytes: the LDS of the
// fused contraction's group sums (0: prolongate-to-fine), which reuse the place of the V tile
static void vector_kernel_launch(const TransferGeom &g, int precision, int NV, size_t redBytes, bool *staged, int *threads, int *workgroups,
                                 size_t *ldsBytes) {
  const size_t tileBytes = prolong_tile_lds(precision, NV);
  *staged = tileBytes <= kTransferMaxLds;  // (not: fp64, n_vec > 53)
  *threads = kPrTile * kPrGroups;
  *workgroups = 2 * ((g.volumeCB + kPrTile - 1) / kPrTile);
  *ldsBytes = *staged ? std::max(tileBytes, redBytes) : redBytes;
}

ProlongForm select_prolong_form(const MugiqHipTransfer &T, int finePrecision, int fineOrder, int nVec, const TransferSwitches &sw) {
  ProlongForm f;
  const TransferGeom &g = f.geom = transfer_geom(T);
  const int NV = T.nVec, blocks = (nVec + 7) / 8;
  f.precision = finePrecision, f.order = fineOrder;
  f.workspaceBytes = (size_t)16 * (2 * (size_t)g.volumeCBc) * 2 * (size_t)NV * (size_t)(8 * blocks);  // [coarse site][chi][j][n] fp64 complex
  // the matrix pipe: fp64 FLOAT2 fine fields, n_vec 8 | 16 | 24 (two V tiles fit the LDS), aggregates of a multiple of 16 sites
  if (finePrecision == 8 && fineOrder == 2 && (NV == 8 || NV == 16 || NV == 24) && sw.prolongMfma && g.aggVol % kCmS == 0) {
    f.family = MUGIQ_HIP_PROLONG_FAMILY_MFMA;
    f.threads = 64 * kPmWaves;
    f.workgroups = 2 * g.volumeCBc;  // one per aggregate
    f.ldsBytes = 2 * congruence_mfma_tile_lds(NV);
    // passes: a workgroup keeps 4 * kPmPairs blocks of eight eigenvectors per chirality resident; more eigenvectors than that are
    // split evenly (V is staged once per pass: 12 n_vec 16 B per site against 192 B per site and eigenvector written)
    f.passes = (blocks + sw.passBlocks - 1) / sw.passBlocks;
    f.blocksPerPass = (blocks + f.passes - 1) / f.passes;
    return f;
  }
  bool staged;
  vector_kernel_launch(g, finePrecision, NV, 0, &staged, &f.threads, &f.workgroups, &f.ldsBytes);
  f.family = staged ? MUGIQ_HIP_PROLONG_FAMILY_VECTOR_STAGED : MUGIQ_HIP_PROLONG_FAMILY_VECTOR_GLOBAL;
  return f;
}

ContractForm select_prolong_contract_form(const MugiqHipTransfer &T, int loopPrecision, int nVec, const TransferSwitches &sw) {
  ContractForm f;
  const TransferGeom &g = f.geom = transfer_geom(T);
  const int NV = T.nVec, P = T.precision;
  f.precision = P, f.loopPrecision = loopPrecision;
  // The coarse-grid plan: n_vec = 8, 16, 32 (chunks of 8 columns) and 12, 24 (chunks of 12); NH = n_vec / chunk lanes per
  // (site, chi, chi') must be a power of two (shuffle reduction) and 4 * NH * SPR <= 1024 threads.  (6-column chunks on 16 lanes per
  // site measured 8 % slower.)  SPR = 64 sites per round where the LDS allows, else 32
  const int JC = NV % 12 == 0 ? 12 : 8, NH = NV / JC;
  int SPR = 64;
  if (congruence_lds(P, loopPrecision, NV, SPR) > 150 * 1024 || 4 * NH * SPR > 1024) SPR = 32;
  if (sw.mgPlan && (NV == 8 || NV == 16 || NV == 32 || NV == 12 || NV == 24) && congruence_lds(P, loopPrecision, NV, SPR) <= 150 * 1024) {
    f.workgroups = 2 * g.volumeCBc;  // one per aggregate
    f.outerB = (2 * NV + 15) / 16;
    f.tableBytes = align256(sizeof(void *) * (size_t)nVec + (size_t)loopPrecision * nVec);
    f.scratchBytes = f.tableBytes + (size_t)2 * loopPrecision * (2 * (size_t)g.volumeCBc) * (2 * NV) * (2 * NV);
    // fp64 accumulation, n_vec = 8, 16, 24, 32, aggregates of a multiple of 16 sites: the congruence on the matrix pipe
    if (loopPrecision == 8 && (NV == 8 || NV == 16 || NV == 24 || NV == 32) && g.aggVol % kCmS == 0 && sw.mgMfma) {
      f.family = MUGIQ_HIP_CONTRACT_FAMILY_COARSE_MFMA;
      f.glds = congruence_mfma_glds(P, NV);
      f.threads = 64 * (NV / 2);
      f.ldsBytes = (f.glds ? 2 : 1) * congruence_mfma_tile_lds(NV) + congruence_mfma_red_lds(NV);
    } else {
      f.family = MUGIQ_HIP_CONTRACT_FAMILY_COARSE_VECTOR;
      f.JC = JC, f.SPR = SPR, f.NH = NH;
      f.threads = 4 * NH * SPR;
      f.ldsBytes = congruence_lds(P, loopPrecision, NV, SPR);
    }
    return f;
  }
  bool staged;
  vector_kernel_launch(g, P, NV, (size_t)loopPrecision * 16 * kPrGroups * kPrTile, &staged, &f.threads, &f.workgroups, &f.ldsBytes);
  f.family = staged ? MUGIQ_HIP_CONTRACT_FAMILY_DIRECT_STAGED : MUGIQ_HIP_CONTRACT_FAMILY_DIRECT_GLOBAL;
  return f;
}

}  // namespace mugiq

extern "C" int mugiq_hip_transfer_form(const MugiqHipTransfer *T, int finePrecision, int fineOrder, int loopPrecision, int nVec,
                                       MugiqHipTransferForm *out) {
  using namespace mugiq;
  const char *who = "mugiq_hip_transfer_form";
  if (!T || !out || nVec < 1) return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: NULL argument or nVec = %d < 1", who, nVec);
  // the transfer-shape checks of the compute calls, against the coarse fields the library would lay out itself
  MugiqHipCoarseField c = coarse_side_layout(*T);
  c.data = out;  // (any non-NULL value: never read)
  if (int st = validate_transfer(T, &c, who)) return st;
  if (finePrecision == 0) finePrecision = T->precision;
  if (loopPrecision == 0) loopPrecision = T->precision;
  if (finePrecision != T->precision || (fineOrder != 2 && fineOrder != 4))
    return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: fine precision %d (transfer: %d), field order %d", who, finePrecision, T->precision, fineOrder);
  if (!(loopPrecision == T->precision || (loopPrecision == 8 && T->precision == 4)))
    return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: loop precision %d with field precision %d is not supported", who, loopPrecision, T->precision);
  const TransferSwitches sw = transfer_switches_from_env();
  const ProlongForm p = select_prolong_form(*T, finePrecision, fineOrder, nVec, sw);
  const ContractForm q = select_prolong_contract_form(*T, loopPrecision, nVec, sw);
  memset(out, 0, sizeof(*out));
  for (int d = 0; d < 4; d++) out->X[d] = p.geom.X[d], out->Xc[d] = p.geom.Xc[d], out->bs[d] = p.geom.bs[d];
  out->aggVol = p.geom.aggVol, out->volumeCB = p.geom.volumeCB, out->volumeCBc = p.geom.volumeCBc;
  out->coarseNColor = c.nColor, out->coarseStride = c.stride, out->coarseParityOffset = (long long)c.parity_offset;
  out->prolongFamily = p.family, out->prolongThreads = p.threads, out->prolongWorkgroups = p.workgroups;
  out->prolongPasses = p.passes, out->prolongBlocksPerPass = p.blocksPerPass;
  out->prolongLdsBytes = (long long)p.ldsBytes, out->prolongWorkspaceBytes = (long long)p.workspaceBytes;
  out->contractFamily = q.family, out->contractThreads = q.threads, out->contractWorkgroups = q.workgroups;
  out->JC = q.JC, out->SPR = q.SPR, out->NH = q.NH, out->outerB = q.outerB, out->glds = q.glds;
  out->contractLdsBytes = (long long)q.ldsBytes, out->contractScratchBytes = (long long)q.scratchBytes;
  return MUGIQ_HIP_SUCCESS;
}
