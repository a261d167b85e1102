// The plan of a compute of the loop driver (csrc/loop_driver.cpp): what happens to every displacement entry, in which order, and which
// buffers that takes -- decided once, on the host, from descriptors alone.  make_loop_plan makes no HIP call and touches no device
// memory; the driver and the query mugiq_hip_loop_plan both go through it, so what the query reports is what runs.
#pragma once
#include <vector>

#include "internal.h"

namespace mugiq {

struct LoopPlanInput {
  int nEntries = 0, nLoop = 1;                // the entry table; nLoop = 1 + the lengths of all entries
  const int *dir = nullptr, *sign = nullptr, *start = nullptr, *stop = nullptr;
  const MugiqHipSpinorField *ev = nullptr;    // geometry only
  int nEv = 0, precision = 8, loopPrecision = 8;
  bool twoSided = false, coarseMode = false;
  const MugiqHipGaugeField *gauge = nullptr;  // precision and R[4] only; may be NULL without entries
  int commDim[4] = {0, 0, 0, 0}, grid[4] = {1, 1, 1, 1};
  bool haveComm = false, groupCallbacks = false;
  bool axialOk[4] = {true, true, true, true};
  const int *momMatrix = nullptr;
  int Nmom = 0, calcType = MUGIQ_HIP_LOOP_CALC_TYPE_OPT_KERNEL;
  bool doMomProj = false, momProjDone = false;
  size_t deviceBytes = 0;  // total memory of the device (hipMemGetInfo): the same on every rank, unlike the free memory
};

struct EntryPlan : MugiqHipLoopEntryPlan {  // (the members of include/mugiq_hip.h)
  std::vector<int> kv;                      // the lengths start .. stop
  FusedForm form;                           // route FUSED: the kernel form of its fused calls (csrc/fused_form.h)
};

struct LoopPlan {
  std::vector<EntryPlan> entry;
  std::vector<int> order;      // -1: the ultra-local loop
  int earlyEntry = -2;         // the entry that runs before the halos are packed (-2: none)
  int earlyPackRoom = 0;       // > 0: the halos are prepared before that entry runs (it may write this many of their face layers)
  bool postHalos = false, carryUltra = false, momReflect = false, grouped = false;
  std::vector<int> packTargets;  // the posted entries whose face layers the early entry writes (from entry[id].entryPacksFrom on)
  std::vector<size_t> reserve;   // what the scratch pool must hold before the compute, in the order it is reserved
};

LoopPlan make_loop_plan(const LoopPlanInput &in);
// can the fused reorder + x step of the momentum projection take this lattice?  (else: reorder, then the three separable steps)
bool fused_projection_applies(int loopPrecision, const int localL[4], int nData, const int *momMatrix, int Nmom);

}  // namespace mugiq
