// make_loop_plan: every decision the loop driver (csrc/loop_driver.cpp) takes about a displacement entry, taken once.  Host only.
// The driver's environment switches (MUGIQ_HIP_HALO_AHEAD, _REFLECT, _REFLECT_MOM, _SELF_HALO_COPY, _HALO_BLOCKS, _CARRY_ULTRALOCAL)
// are read here and nowhere else in the driver.  Nothing in the plan may depend on what can differ between ranks (such as the memory
// free right now): every rank has to take the same decisions, or the transfers would not pair up.
#include "loop_plan.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mugiq {

static bool env_is(const char *name, bool zero) {  // the switch is set, and to zero / to something else
  const char *e = getenv(name);
  return e && (atoi(e) == 0) == zero;
}
static int ceil_div(int a, int b) { return (a + b - 1) / b; }

bool fused_projection_applies(int loopPrecision, const int localL[4], int nData, const int *momMatrix, int Nmom) {
  std::vector<int> px;
  for (int n = 0; n < Nmom; n++)
    if (std::find(px.begin(), px.end(), momMatrix[3 * n]) == px.end()) px.push_back(momMatrix[3 * n]);
  return eo_dft_x_time_chunk(loopPrecision, localL, (int)px.size()) >= 1 && localL[2] <= 65535 && nData <= 65535;
}

// One OPT entry.  budget: what is left of the quarter of the device memory the ghost-layer buffers posted ahead may take.
static void plan_opt_entry(const LoopPlanInput &in, LoopPlan &P, int id, size_t &budget, const FusedSwitches &sw) {
  EntryPlan &e = P.entry[id];
  const MugiqHipSpinorField &ev = *in.ev;
  const int dir = in.dir[id], sign = in.sign[id], start = in.start[id], stop = in.stop[id];
  // Reflected (csrc/reflect.hip): from an entry computed earlier with the same direction, the opposite sign and all of its lengths.
  // Not two-sided (L^-(x) = eta conj L^+(x - k mu) rests on the left and right vectors being the same), and not past the nearest
  // neighbour of a partitioned direction: one halo of the source slot cannot serve that
  const bool past = e.part && stop > ev.X[dir];
  if (!in.twoSided && !past && !env_is("MUGIQ_HIP_REFLECT", true))
    for (int jd = 0; jd < id && e.derivedFrom < 0; jd++)
      if (in.dir[jd] == dir && in.sign[jd] != sign && in.start[jd] <= start && stop <= in.stop[jd] && P.entry[jd].derivedFrom < 0) e.derivedFrom = jd;
  e.route = MUGIQ_HIP_LOOP_ROUTE_REFLECTED, e.kernel = MUGIQ_HIP_ENTRY_KERNEL_REFLECTED;
  if (e.derivedFrom >= 0) return;
  // the kernel form of its fused calls (the driver holds the gauge of a matrix-pipe entry, or its lengths start at 1)
  e.form = select_fused_form(ev, dir, e.kv.data(), e.nK, e.part, true, in.twoSided, in.loopPrecision, sw, e.tile != 0);
  // Step by step: a length past the nearest neighbour (the multi-layer halo cannot reach there, single steps can); for two-sided loops
  // also every entry the two-sided matrix-pipe tile does not take (lengths > 8, a partitioned x axis, no tile geometry, tile refused)
  if (past || e.form.family == MUGIQ_HIP_FUSED_FAMILY_NONE) {
    e.route = MUGIQ_HIP_LOOP_ROUTE_STEPWISE, e.kernel = MUGIQ_HIP_ENTRY_KERNEL_STEPWISE, e.needsMemset = 1;
    const size_t fieldB = (size_t)2 * ev.parity_offset * 2 * (size_t)in.precision, aux = (size_t)8 << 30;  // two auxiliary fields per eigenvector
    e.blockN = (int)std::max<size_t>(1, std::min<size_t>((size_t)in.nEv, aux / (2 * fieldB)));
    e.nBlocks = ceil_div(in.nEv, e.blockN);
    return;
  }
  e.route = MUGIQ_HIP_LOOP_ROUTE_FUSED, e.kernel = e.form.kernel;
  // an axis of extent 1 that is partitioned all the same: the rank is its own neighbour, the face layers are packed straight into the
  // ghost buffer -- no send buffer, no message (MUGIQ_HIP_SELF_HALO_COPY=1: keep them)
  e.selfAlias = e.part && in.haveComm && in.grid[dir] == 1 && !env_is("MUGIQ_HIP_SELF_HALO_COPY", false);
  e.ahead = e.part && 2 * (size_t)e.haloBytes <= budget;  // (else it exchanges eigenvector blocks of <= 4 GiB inside its own turn)
  if (e.ahead) budget -= 2 * (size_t)e.haloBytes;
  // Its links: the axial gauge (csrc/fused_mfma.hip) straight from the gauge field where that reaches far enough -- a partitioned entry
  // only when its halo is posted -- else the path-link fields W_0 .. W_stop, and from them the gauge once for all launches of a posted
  // entry, and where the lengths do not start at 1 (the links of the call then do not hold W_1); otherwise every fused call builds its own
  e.gaugeBytes = (long long)e.form.gaugeBytes;
  e.gaugeFromField = e.gaugeBytes && (e.ahead || !e.part) && axial_gauge_from_links_possible(ev, *in.gauge, stop, dir, sign, sw);
  if (!e.gaugeFromField) {
    e.nLinkFields = stop + 1;
    e.buildGaugeFromLinks = e.gaugeBytes && (e.ahead || start > 1);
  }
  // Blocks of eigenvectors.  A posted halo travels in blocks of about 2 GiB (at most 8): the first is on its way after a fraction of the
  // packing, and the boundary tiles of the first blocks run while the last ones still travel (MUGIQ_HIP_HALO_BLOCKS fixes the number).
  // A partitioned entry that is not posted is bounded by ghost buffers of 4 GiB per direction.
  e.blockN = in.nEv;
  if (e.ahead) {
    int nb = (int)std::min<size_t>(8, std::max<size_t>(1, ((size_t)e.haloBytes + ((size_t)1 << 31) - 1) >> 31));
    if (e.selfAlias) nb = 1;  // nothing travels: one block, one launch of the boundary tiles
    if (const char *s = getenv("MUGIQ_HIP_HALO_BLOCKS")) nb = std::max(1, std::min(64, atoi(s)));
    e.blockN = ceil_div(in.nEv, std::min(nb, in.nEv));
  } else if (e.part) {
    e.blockN = (int)std::max<size_t>(1, std::min<size_t>((size_t)in.nEv, ((size_t)4 << 30) / (size_t)e.perVecHaloBytes));
  }
  e.nBlocks = ceil_div(in.nEv, e.blockN);
}

LoopPlan make_loop_plan(const LoopPlanInput &in) {
  LoopPlan P;
  const int n = in.nEntries;
  const bool basic = in.calcType == MUGIQ_HIP_LOOP_CALC_TYPE_BASIC_KERNEL;
  const size_t cplx = 2 * (size_t)in.precision;
  P.entry.resize(n);
  size_t budget = env_is("MUGIQ_HIP_HALO_AHEAD", true) ? 0 : in.deviceBytes / 4;
  const FusedSwitches sw = fused_switches_from_env();
  bool anyDerived = false;
  for (int id = 0; id < n; id++) {
    EntryPlan &e = P.entry[id];  // (zeroed by resize)
    const int dir = in.dir[id];
    e.derivedFrom = e.entryPacksFrom = -1;
    e.part = in.commDim[dir] != 0;
    e.high = in.sign[id] == MUGIQ_HIP_DISP_SIGN_PLUS ? 0 : 1;  // sign +: my LOW face feeds the backward neighbour
    e.kStart = in.start[id], e.nK = in.stop[id] - in.start[id] + 1;
    for (int k = in.start[id]; k <= in.stop[id]; k++) e.kv.push_back(k);
    e.tile = in.axialOk[dir];
    e.faceBytes = (long long)((size_t)24 * (in.ev->volumeCB / in.ev->X[dir]) * cplx);
    e.perVecHaloBytes = in.stop[id] * e.faceBytes;  // `stop` face layers of one eigenvector
    e.haloBytes = e.perVecHaloBytes * in.nEv;
    if (basic) e.route = MUGIQ_HIP_LOOP_ROUTE_STEPWISE, e.kernel = MUGIQ_HIP_ENTRY_KERNEL_STEPWISE, e.needsMemset = 1;  // the reference's own sequence: nothing derived, nothing posted
    else plan_opt_entry(in, P, id, budget, sw);
    anyDerived = anyDerived || e.derivedFrom >= 0;
    P.postHalos = P.postHalos || e.ahead;
  }
  // The order.  The slots are independent, so the order of lib/loop_mugiq.cpp:455 is kept for BASIC only; OPT runs the ultra-local loop
  // and the entries of unpartitioned directions while the halos travel, then the partitioned entries, and the reflected entries last.
  P.order.push_back(-1);
  for (int pass = 0; pass < 3; pass++)
    for (int id = 0; id < n; id++) {
      const bool derived = P.entry[id].derivedFrom >= 0, part = P.entry[id].part;
      if (basic ? pass == 0 : (pass == 0 && !derived && !part) || (pass == 1 && !derived && part) || (pass == 2 && derived)) P.order.push_back(id);
    }
  if (basic) return P;
  // the ultra-local loop may ride along with a displaced entry (MUGIQ_HIP_CARRY_ULTRALOCAL=0: never): it then moves to the end of the
  // order and is skipped if some entry has taken it along
  P.carryUltra = n > 0 && !in.coarseMode && !env_is("MUGIQ_HIP_CARRY_ULTRALOCAL", true);
  if (P.carryUltra) std::rotate(P.order.begin(), P.order.begin() + 1, P.order.end());
  // momentum-space output only needs the reflected entries in momentum space (csrc/reflect_mom.cpp): when the momentum list holds -p
  // for every p they are left out of position space and derived on the gathered array (MUGIQ_HIP_REFLECT_MOM=0: never)
  std::vector<int> neg;
  P.momReflect = in.doMomProj && !in.momProjDone && anyDerived && !env_is("MUGIQ_HIP_REFLECT_MOM", true) &&
                 fused_projection_applies(in.loopPrecision, in.ev->X, 16 * in.nLoop, in.momMatrix, in.Nmom) &&
                 momenta_negation_table(in.momMatrix, in.Nmom, neg);
  P.grouped = in.haveComm && in.groupCallbacks;
  if (!P.postHalos) return P;
  // one entry that needs no halo goes FIRST, before the halos are packed (see post_halos in the driver) ...
  for (int id : P.order)
    if (id >= 0 && P.entry[id].derivedFrom < 0 && !P.entry[id].part) {
      P.earlyEntry = id;
      break;
    }
  // ... and where it is a mu = x entry on the row tile of csrc/fused_mfma.hip and the partitioned axes are z / t, it writes the face
  // layers itself (two-sided: pack kernels), but for the first block of a halo that really travels: that goes out ahead
  if (P.earlyEntry >= 0 && in.dir[P.earlyEntry] == 0 && in.loopPrecision == in.precision && !in.twoSided) {
    const EntryPlan &early = P.entry[P.earlyEntry];
    P.earlyPackRoom = early.form.packCapacity;
    for (int id = 0; id < n && (int)P.packTargets.size() < P.earlyPackRoom; id++) {
      EntryPlan &e = P.entry[id];
      const int from = e.selfAlias ? 0 : e.blockN;
      if (!e.ahead || in.dir[id] < 2 || from >= in.nEv) continue;
      e.entryPacksFrom = from;
      P.packTargets.push_back(id);
    }
  }
  // What the pool holds before the compute (hipMalloc of multi-GB buffers costs ~40 ms per GB, so they are allocated with the loop
  // object): per posted entry its link fields with their two face buffers, its ghost and send buffers and its gauge ...
  const size_t fieldB = (size_t)24 * in.ev->volumeCB * cplx;  // a FLOAT2 pad-0 path-link field
  for (const EntryPlan &e : P.entry) {
    if (!e.ahead) continue;
    P.reserve.insert(P.reserve.end(), e.nLinkFields, fieldB);  // E_0 .. E_stop, held until the entry has run
    if (e.nLinkFields) P.reserve.insert(P.reserve.end(), 2, (size_t)e.faceBytes);
    P.reserve.insert(P.reserve.end(), e.selfAlias ? 1 : 2, (size_t)e.haloBytes);
    if (e.gaugeBytes) P.reserve.push_back((size_t)e.gaugeBytes);
  }
  // ... and the links of the early entry, which stay out of the pool until the compute ends: they come on top
  if (P.earlyEntry >= 0) {
    const EntryPlan &e = P.entry[P.earlyEntry];
    if (e.gaugeFromField) P.reserve.push_back((size_t)e.gaugeBytes);
    else P.reserve.insert(P.reserve.end(), in.stop[P.earlyEntry] + 1, fieldB);
  }
  return P;
}

}  // namespace mugiq

extern "C" int mugiq_hip_loop_plan(const MugiqHipLoopParam *p, const MugiqHipSpinorField *eVec, int nEv, int twoSided, int coarseMode,
                                   const MugiqHipComm *comm, const int axialOk[4], size_t deviceBytes, MugiqHipLoopPlan *out) {
  using namespace mugiq;
  const char *who = "mugiq_hip_loop_plan";
  MUGIQ_REQUIRE(p && eVec && axialOk && out && nEv >= 1, "%s: NULL argument or nEv < 1", who);
  const int n = p->doNonLocal ? p->nDispEntries : 0;
  MUGIQ_REQUIRE(n >= 0 && n <= MUGIQ_HIP_LOOP_PLAN_MAX_ENTRIES, "%s: %d displacement entries (at most %d)", who, n, MUGIQ_HIP_LOOP_PLAN_MAX_ENTRIES);
  MUGIQ_REQUIRE(n == 0 || (p->disp_str && p->disp_start && p->disp_stop && p->gauge), "%s: entries need their table and the gauge descriptor", who);
  MUGIQ_REQUIRE(!p->doMomProj || (p->Nmom >= 1 && p->momMatrix), "%s: doMomProj needs a momentum list", who);
  for (int d = 0; d < 4; d++) MUGIQ_REQUIRE(eVec->X[d] > 0 && eVec->volumeCB > 0, "%s: eVec carries no geometry", who);
  std::vector<int> dir(n), sign(n), start(n), stop(n);
  LoopPlanInput in;
  for (int id = 0; id < n; id++) {  // (the table as mugiq_hip_loop_create reads it)
    if (int st = mugiq_hip_parse_displacement(p->disp_str[id], &dir[id], &sign[id])) return st;
    start[id] = std::min(p->disp_start[id], p->disp_stop[id]);
    stop[id] = std::max(p->disp_start[id], p->disp_stop[id]);
    MUGIQ_REQUIRE(start[id] >= 1, "%s: displacement lengths must be >= 1 (entry %d: %d)", who, id, start[id]);
    in.nLoop += stop[id] - start[id] + 1;
  }
  in.nEntries = n;
  in.dir = dir.data(), in.sign = sign.data(), in.start = start.data(), in.stop = stop.data();
  in.ev = eVec, in.nEv = nEv, in.precision = eVec->precision;
  in.loopPrecision = p->loopPrecision ? p->loopPrecision : eVec->precision;
  in.twoSided = twoSided != 0, in.coarseMode = coarseMode != 0;
  in.gauge = p->gauge;
  in.haveComm = comm != nullptr, in.groupCallbacks = comm && comm->group_begin && comm->group_end;
  for (int d = 0; d < 4; d++) in.commDim[d] = comm_partitioned(comm, d), in.grid[d] = comm ? comm->grid[d] : 1, in.axialOk[d] = axialOk[d] != 0;
  in.doMomProj = p->doMomProj != 0, in.momMatrix = p->momMatrix, in.Nmom = p->Nmom;
  in.calcType = p->calcType, in.deviceBytes = deviceBytes;
  const LoopPlan P = make_loop_plan(in);
  MUGIQ_REQUIRE(P.reserve.size() <= MUGIQ_HIP_LOOP_PLAN_MAX_BUFFERS, "%s: %zu buffers to reserve (at most %d are reported)", who, P.reserve.size(),
                MUGIQ_HIP_LOOP_PLAN_MAX_BUFFERS);
  memset(out, 0, sizeof(*out));
  out->nEntries = n, out->nOrder = (int)P.order.size(), out->nPackTargets = (int)P.packTargets.size(), out->nReserve = (int)P.reserve.size();
  out->earlyEntry = P.earlyEntry, out->carryUltra = P.carryUltra, out->momReflect = P.momReflect, out->grouped = P.grouped;
  std::copy(P.order.begin(), P.order.end(), out->order);
  std::copy(P.packTargets.begin(), P.packTargets.end(), out->packTargets);
  std::copy(P.reserve.begin(), P.reserve.end(), out->reserve);
  std::copy(P.entry.begin(), P.entry.end(), out->entry);  // (the members of the C struct)
  return MUGIQ_HIP_SUCCESS;
}
