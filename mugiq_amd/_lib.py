"""ctypes loader for libmugiq_hip.so (built in-tree by `make -C mugiq_amd/csrc` / __graft_entry__.build()).

There is NO fallback: if the HIP library is missing or a call fails, an exception is raised.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MUGIQ_HIP_LIB selects another build of the same library (e.g. a diagnostic build); never a different backend
LIB_PATH = os.environ.get("MUGIQ_HIP_LIB") or os.path.join(_HERE, "libmugiq_hip.so")


class MugiqHipError(RuntimeError):
    """Raised for every non-zero status of the C ABI (the reference aborts through errorQuda)."""


class SpinorDesc(ctypes.Structure):
    """MugiqHipSpinorField (include/mugiq_hip.h)."""
    _fields_ = [("data", ctypes.c_void_p),
                ("precision", ctypes.c_int),
                ("field_order", ctypes.c_int),
                ("nParity", ctypes.c_int),
                ("volumeCB", ctypes.c_int),
                ("stride", ctypes.c_int),
                ("X", ctypes.c_int * 4),
                ("parity_offset", ctypes.c_int64),
                ("ghost", (ctypes.c_void_p * 2) * 4)]


class GaugeDesc(ctypes.Structure):
    """MugiqHipGaugeField (include/mugiq_hip.h)."""
    _fields_ = [("data", ctypes.c_void_p),
                ("precision", ctypes.c_int),
                ("X", ctypes.c_int * 4),
                ("R", ctypes.c_int * 4),
                ("stride", ctypes.c_int),
                ("parity_offset", ctypes.c_int64)]


class CloverDesc(ctypes.Structure):
    """MugiqHipCloverField (include/mugiq_hip.h)."""
    _fields_ = [("data", ctypes.c_void_p),
                ("precision", ctypes.c_int),
                ("X", ctypes.c_int * 4),
                ("volumeCB", ctypes.c_int),
                ("stride", ctypes.c_int),
                ("parity_offset", ctypes.c_int64)]


class CoarseDesc(ctypes.Structure):
    """MugiqHipCoarseField (include/mugiq_hip.h)."""
    _fields_ = [("data", ctypes.c_void_p), ("precision", ctypes.c_int), ("nSpin", ctypes.c_int), ("nColor", ctypes.c_int),
                ("volumeCB", ctypes.c_int), ("stride", ctypes.c_int), ("X", ctypes.c_int * 4), ("parity_offset", ctypes.c_int64)]


class TransferDesc(ctypes.Structure):
    """MugiqHipTransfer (include/mugiq_hip.h)."""
    _fields_ = [("V", ctypes.c_void_p), ("precision", ctypes.c_int), ("nVec", ctypes.c_int), ("geoBlockSize", ctypes.c_int * 4),
                ("spinBlockSize", ctypes.c_int), ("X", ctypes.c_int * 4), ("stride", ctypes.c_int), ("parity_offset", ctypes.c_int64)]


class CoarseOperatorDesc(ctypes.Structure):
    """MugiqHipCoarseOperator (include/mugiq_hip.h)."""
    _fields_ = [("data", ctypes.c_void_p), ("precision", ctypes.c_int), ("nVec", ctypes.c_int), ("X", ctypes.c_int * 4), ("volumeCB", ctypes.c_int),
                ("kappa", ctypes.c_double), ("hasClover", ctypes.c_int)]


class CoarseHaloDesc(ctypes.Structure):
    """MugiqHipCoarseHalo (include/mugiq_hip.h)."""
    _fields_ = [("Yback", ctypes.c_void_p * 4), ("Yfwd", ctypes.c_void_p * 4), ("precision", ctypes.c_int), ("nVec", ctypes.c_int),
                ("X", ctypes.c_int * 4), ("volumeCB", ctypes.c_int), ("dims", ctypes.c_int * 4)]


class MgSolveParam(ctypes.Structure):
    """MugiqHipMgSolveParam (include/mugiq_hip.h)."""
    _fields_ = [("tol", ctypes.c_double), ("maxIter", ctypes.c_int), ("nKrylov", ctypes.c_int), ("nuPre", ctypes.c_int), ("nuPost", ctypes.c_int),
                ("omega", ctypes.c_double), ("coarseIters", ctypes.c_int)]


class CoarseDeflationDesc(ctypes.Structure):
    """MugiqHipCoarseDeflation (include/mugiq_hip.h)."""
    _fields_ = [("nEv", ctypes.c_int), ("W", ctypes.POINTER(CoarseDesc)), ("U", ctypes.POINTER(CoarseDesc)), ("sigma", ctypes.POINTER(ctypes.c_double))]


class BlockOrthoInfo(ctypes.Structure):
    """MugiqHipBlockOrthoInfo (include/mugiq_hip.h)."""
    _fields_ = [("minPivotRatio", ctypes.c_double), ("zeroColumns", ctypes.c_int)]


class MgSetupParam(ctypes.Structure):
    """MugiqHipMgSetupParam (include/mugiq_hip.h)."""
    _fields_ = [("setupMaxIter", ctypes.c_int), ("setupTol", ctypes.c_double), ("nBlockOrtho", ctypes.c_int), ("rankTol", ctypes.c_double),
                ("refineCycles", ctypes.c_int), ("refineIters", ctypes.c_int)]


class MgSetupInfo(ctypes.Structure):
    """MugiqHipMgSetupInfo (include/mugiq_hip.h)."""
    _fields_ = [("cgIters", ctypes.c_int * 64), ("minPivotRatio", ctypes.c_double), ("zeroColumns", ctypes.c_int), ("orthonormality", ctypes.c_double),
                ("hostReads", ctypes.c_int), ("cgHostReadsEstimate", ctypes.c_int)]


class CoarseEigParam(ctypes.Structure):
    """MugiqHipCoarseEigParam (include/mugiq_hip.h)."""
    _fields_ = [("nConv", ctypes.c_int), ("nKr", ctypes.c_int), ("tol", ctypes.c_double), ("maxIter", ctypes.c_int), ("polyDeg", ctypes.c_int),
                ("aMin", ctypes.c_double), ("aMax", ctypes.c_double), ("nOrtho", ctypes.c_int), ("rankTol", ctypes.c_double)]


class CoarseEigInfo(ctypes.Structure):
    """MugiqHipCoarseEigInfo (include/mugiq_hip.h)."""
    _fields_ = [("iters", ctypes.c_int), ("nConverged", ctypes.c_int), ("opBlocks", ctypes.c_int), ("aMaxUsed", ctypes.c_double),
                ("aMinLast", ctypes.c_double), ("orthonormality", ctypes.c_double), ("hostReads", ctypes.c_int), ("hostDenseSeconds", ctypes.c_double)]


class CoarseEigGridInfo(ctypes.Structure):
    """MugiqHipCoarseEigGridInfo (include/mugiq_hip.h)."""
    _fields_ = [("exchanges", ctypes.c_int), ("rankSums", ctypes.c_int), ("packLaunches", ctypes.c_int), ("stepPacked", ctypes.c_int)]


class MgSolveGridInfo(ctypes.Structure):
    """MugiqHipMgSolveGridInfo (include/mugiq_hip.h)."""
    _fields_ = [("fineExchanges", ctypes.c_int), ("coarseExchanges", ctypes.c_int), ("rankSums", ctypes.c_int), ("rankSumMessages", ctypes.c_int)]


class ProjectPlan(ctypes.Structure):
    """MugiqHipProjectPlan (include/mugiq_hip.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("form", "nks", "mb", "nPx", "tChunk", "nChunks", "lastChunk", "tiles", "tilesPerWg",
                                            "workgroupsX", "rowPasses", "pxPasses", "stagingPieces", "redOffset")] + \
               [("ldsBytes", ctypes.c_longlong)]


LOOP_PLAN_MAX_ENTRIES, LOOP_PLAN_MAX_BUFFERS = 64, 512


class LoopEntryPlan(ctypes.Structure):
    """MugiqHipLoopEntryPlan (include/mugiq_hip.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("derivedFrom", "route", "part", "high", "kStart", "nK", "tile", "gaugeFromField", "nLinkFields",
                                            "buildGaugeFromLinks", "ahead", "selfAlias", "nBlocks", "blockN", "needsMemset", "entryPacksFrom",
                                            "kernel")] + \
               [(n, ctypes.c_longlong) for n in ("faceBytes", "haloBytes", "perVecHaloBytes", "gaugeBytes")]


class FusedForm(ctypes.Structure):
    """MugiqHipFusedForm (include/mugiq_hip.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("kernel", "family", "slotsPerLaunch", "packCapacity")] + [("gaugeBytes", ctypes.c_longlong)] + \
               [(n, ctypes.c_int) for n in ("nSlots", "kmax", "waves", "staged", "tj", "lines", "rowGroups", "rows", "rowChunk", "leftBufElems",
                                            "ph", "glds", "npc", "np", "m", "phl")] + [("ldsBytes", ctypes.c_longlong)]


class TransferForm(ctypes.Structure):
    """MugiqHipTransferForm (include/mugiq_hip.h)."""
    _fields_ = [(n, ctypes.c_int * 4) for n in ("X", "Xc", "bs")] + \
               [(n, ctypes.c_int) for n in ("aggVol", "volumeCB", "volumeCBc", "coarseNColor", "coarseStride")] + [("coarseParityOffset", ctypes.c_longlong)] + \
               [(n, ctypes.c_int) for n in ("prolongFamily", "prolongThreads", "prolongWorkgroups", "prolongPasses", "prolongBlocksPerPass")] + \
               [(n, ctypes.c_longlong) for n in ("prolongLdsBytes", "prolongWorkspaceBytes")] + \
               [(n, ctypes.c_int) for n in ("contractFamily", "contractThreads", "contractWorkgroups", "JC", "SPR", "NH", "outerB", "glds")] + \
               [(n, ctypes.c_longlong) for n in ("contractLdsBytes", "contractScratchBytes")]


class LoopPlan(ctypes.Structure):
    """MugiqHipLoopPlan (include/mugiq_hip.h)."""
    _fields_ = [(n, ctypes.c_int) for n in ("nEntries", "nOrder", "nPackTargets", "nReserve", "earlyEntry", "carryUltra", "momReflect", "grouped")] + \
               [("order", ctypes.c_int * (LOOP_PLAN_MAX_ENTRIES + 1)), ("packTargets", ctypes.c_int * LOOP_PLAN_MAX_ENTRIES),
                ("reserve", ctypes.c_longlong * LOOP_PLAN_MAX_BUFFERS), ("entry", LoopEntryPlan * LOOP_PLAN_MAX_ENTRIES)]


_I4 = ctypes.POINTER(ctypes.c_int)
_VP = ctypes.c_void_p
_SP = ctypes.POINTER(SpinorDesc)
_GP = ctypes.POINTER(GaugeDesc)
_CP = ctypes.POINTER(CloverDesc)

# name -> (restype, argtypes); every symbol include/mugiq_hip.h declares
SIGNATURES = {
    "mugiq_hip_version": (ctypes.c_int, []),
    "mugiq_hip_last_error": (ctypes.c_char_p, []),
    "mugiq_hip_device_count": (ctypes.c_int, []),
    "mugiq_hip_release_stream": (ctypes.c_int, [_VP]),
    "mugiq_hip_probe_read_bandwidth": (ctypes.c_int, [_VP, ctypes.c_size_t, ctypes.c_int, _VP]),
    "mugiq_hip_debug_poison_lds": (ctypes.c_int, [_VP]),
    "mugiq_hip_copy_gamma_coeff_to_symbol": (ctypes.c_int, [ctypes.c_int]),
    "mugiq_hip_copy_gamma_map_to_symbol": (ctypes.c_int, [ctypes.c_int]),
    "mugiq_hip_get_gamma_tables": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), _I4,
                                                  ctypes.POINTER(ctypes.c_double), _I4]),
    "mugiq_hip_gamma_name": (ctypes.c_char_p, [ctypes.c_int]),
    "mugiq_hip_perform_loop_contraction": (ctypes.c_int, [_VP, _SP, _SP, ctypes.c_double, _VP]),
    "mugiq_hip_perform_loop_contraction_batched": (ctypes.c_int, [_VP, _SP, _SP, ctypes.POINTER(ctypes.c_double),
                                                                  ctypes.c_int, _VP]),
    "mugiq_hip_perform_loop_contraction_batched_mixed": (ctypes.c_int, [_VP, ctypes.c_int, _SP, _SP, ctypes.POINTER(ctypes.c_double),
                                                                        ctypes.c_int, _VP]),
    "mugiq_hip_displaced_loop_contraction_fused_mixed": (ctypes.c_int, [_VP, ctypes.c_int, _SP, ctypes.POINTER(ctypes.c_double),
                                                                        ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), _I4,
                                                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, _I4, _VP,
                                                                        ctypes.c_int, _VP]),
    "mugiq_hip_displaced_loop_contraction_fused_region": (ctypes.c_int, [_VP, ctypes.c_int, _SP, ctypes.POINTER(ctypes.c_double),
                                                                         ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), _I4,
                                                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, _I4, _VP,
                                                                         ctypes.c_int, ctypes.c_int, _VP]),
    "mugiq_hip_displaced_loop_contraction_fused_carry": (ctypes.c_int, [_VP, ctypes.c_int, _SP, ctypes.POINTER(ctypes.c_double),
                                                                        ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), _I4,
                                                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, _I4, _VP,
                                                                        ctypes.c_int, ctypes.c_int, _VP, _I4, _VP]),
    "mugiq_hip_displaced_loop_contraction_fused_two_sided": (ctypes.c_int, [_VP, ctypes.c_int, _SP, _SP, ctypes.POINTER(ctypes.c_double),
                                                                            ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), _I4,
                                                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, _I4, _VP,
                                                                            ctypes.c_int, ctypes.c_int, _VP, _I4, _VP]),
    "mugiq_hip_perform_covariant_displacement_vector": (ctypes.c_int, [_SP, _SP, _GP, ctypes.c_int, ctypes.c_int,
                                                                       _I4, _VP]),
    "mugiq_hip_pack_face": (ctypes.c_int, [_VP, _SP, ctypes.c_int, ctypes.c_int, _VP]),
    "mugiq_hip_exchange_ghost_vec": (ctypes.c_int, [_SP, _VP, _VP]),
    "mugiq_hip_rccl_get_unique_id": (ctypes.c_int, [_VP]),
    "mugiq_hip_rccl_comm_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _VP, ctypes.c_int, ctypes.c_int, _I4, _I4]),
    "mugiq_hip_rccl_comm_from_nccl": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _VP, _I4, _I4]),
    "mugiq_hip_rccl_comm_fill": (ctypes.c_int, [_VP, _VP]),
    "mugiq_hip_rccl_comm_destroy": (ctypes.c_int, [_VP]),
    "mugiq_hip_rccl_comm_set_multipath": (ctypes.c_int, [_VP, ctypes.c_int]),
    "mugiq_hip_rccl_relay_plan": (ctypes.c_int, [ctypes.c_int, _I4, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, _I4, _I4, _I4,
                                                ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
    "mugiq_hip_alloc_spinor_like": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _I4]),
    "mugiq_hip_free_spinor": (ctypes.c_int, [_SP]),
    "mugiq_hip_copy_spinor": (ctypes.c_int, [_SP, _SP, _VP]),
    "mugiq_hip_zero_spinor": (ctypes.c_int, [_SP, _VP]),
    "mugiq_hip_create_phase_matrix": (ctypes.c_int, [_VP, _I4, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                                     _I4, _I4, _I4, ctypes.c_int, _VP]),
    "mugiq_hip_convert_idx_order_map_gamma": (ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                             ctypes.c_int, _I4, ctypes.c_int, _VP]),
    "mugiq_hip_momentum_projection_workspace": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
                                                                  ctypes.c_int, ctypes.c_int]),
    "mugiq_hip_momentum_projection": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
                                                     ctypes.c_int, ctypes.c_int, _VP, ctypes.c_size_t, _VP]),
    "mugiq_hip_momentum_projection_separable_workspace": (ctypes.c_size_t, [_I4, ctypes.c_int, _I4, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mugiq_hip_momentum_projection_separable": (ctypes.c_int, [_VP, _VP, _I4, ctypes.c_int, ctypes.c_int, _I4, _I4, _I4, ctypes.c_int,
                                                               ctypes.c_int, ctypes.c_int, _VP, ctypes.c_size_t, _VP]),
    "mugiq_hip_convert_and_project": (ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int, _I4, ctypes.c_int, ctypes.c_int, _I4, _I4, _I4,
                                                     ctypes.c_int, _VP, ctypes.c_size_t, _VP]),
    "mugiq_hip_convert_and_project_slots": (ctypes.c_int, [_VP, _VP, ctypes.c_int, _I4, ctypes.c_int, _I4, ctypes.c_int, ctypes.c_int, _I4, _I4, _I4,
                                                           ctypes.c_int, _VP, ctypes.c_size_t, _VP]),
    "mugiq_hip_convert_and_project_plan": (ctypes.c_int, [_I4, ctypes.c_int, _I4, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ProjectPlan)]),
    "mugiq_hip_reflect_momentum_space": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, _I4, ctypes.c_int, _I4, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mugiq_hip_pack_face_layers": (ctypes.c_int, [_VP, _SP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP]),
    "mugiq_hip_reflect_displaced_loop": (ctypes.c_int, [_VP, _VP, _VP, _I4, ctypes.c_int, ctypes.c_int, ctypes.c_int, _I4, ctypes.c_int, _VP]),
    "mugiq_hip_pack_loop_layers": (ctypes.c_int, [_VP, _VP, _I4, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP]),
    "mugiq_hip_displaced_loop_contraction_fused": (ctypes.c_int, [_VP, _SP, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                                                  ctypes.POINTER(ctypes.c_void_p), _I4, ctypes.c_int,
                                                                  ctypes.c_int, ctypes.c_int, _I4, _VP, ctypes.c_int, _VP]),
    "mugiq_hip_deflate_low_modes": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _SP, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int,
                                                   ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    "mugiq_hip_wilson_apply": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, ctypes.c_double, ctypes.c_int, ctypes.c_double, _VP, _VP]),
    "mugiq_hip_compute_evals": (ctypes.c_int, [_SP, ctypes.c_int, _GP, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    "mugiq_hip_project_vector": (ctypes.c_int, [_SP, _SP, _SP, ctypes.c_int, _VP, _VP]),
    "mugiq_hip_wilson_solve": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, ctypes.c_double, _SP, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                              ctypes.c_double, ctypes.c_int, _I4, ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    "mugiq_hip_clover_bytes": (ctypes.c_size_t, [_I4, ctypes.c_int]),
    "mugiq_hip_alloc_clover": (ctypes.c_int, [_CP, _I4, ctypes.c_int]),
    "mugiq_hip_free_clover": (ctypes.c_int, [_CP]),
    "mugiq_hip_compute_clover": (ctypes.c_int, [_CP, _GP, ctypes.c_double, _VP, _VP]),
    "mugiq_hip_exchange_extended_gauge": (ctypes.c_int, [_GP, _VP, _VP]),
    "mugiq_hip_stout_smear": (ctypes.c_int, [_GP, _GP, ctypes.c_double, ctypes.c_int, ctypes.c_int, _VP, _VP]),
    "mugiq_hip_plaquette": (ctypes.c_int, [_GP, ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    "mugiq_hip_wilson_clover_apply": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.c_int, ctypes.c_double, _VP, _VP]),
    "mugiq_hip_compute_evals_clover": (ctypes.c_int, [_SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                                      ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                      ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    "mugiq_hip_compute_evals_coarse": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.c_int, ctypes.POINTER(TransferDesc), ctypes.c_int, _GP, _CP,
                                                      ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                                      ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    "mugiq_hip_coarse_operator_bytes": (ctypes.c_size_t, [_I4, ctypes.c_int, ctypes.c_int]),
    "mugiq_hip_alloc_coarse_operator": (ctypes.c_int, [ctypes.POINTER(CoarseOperatorDesc), _I4, ctypes.c_int, ctypes.c_int]),
    "mugiq_hip_free_coarse_operator": (ctypes.c_int, [ctypes.POINTER(CoarseOperatorDesc)]),
    "mugiq_hip_compute_coarse_operator": (ctypes.c_int, [ctypes.POINTER(CoarseOperatorDesc), ctypes.POINTER(TransferDesc), _GP, _CP, ctypes.c_double,
                                                         _VP, _VP]),
    "mugiq_hip_coarse_apply": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.POINTER(CoarseDesc), ctypes.c_int, ctypes.POINTER(CoarseOperatorDesc),
                                              ctypes.c_int, ctypes.c_double, _VP, _VP]),
    "mugiq_hip_coarse_apply_outputs": (ctypes.c_int, [ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int]),
    "mugiq_hip_compute_evals_coarse_operator": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.c_int, ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int,
                                                               ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                               ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    "mugiq_hip_coarse_halo_bytes": (ctypes.c_size_t, [_I4, ctypes.c_int, ctypes.c_int, _I4]),
    "mugiq_hip_alloc_coarse_halo": (ctypes.c_int, [ctypes.POINTER(CoarseHaloDesc), ctypes.POINTER(CoarseOperatorDesc), _I4]),
    "mugiq_hip_free_coarse_halo": (ctypes.c_int, [ctypes.POINTER(CoarseHaloDesc)]),
    "mugiq_hip_compute_coarse_operator_grid": (ctypes.c_int, [ctypes.POINTER(CoarseOperatorDesc), ctypes.POINTER(CoarseHaloDesc), ctypes.POINTER(TransferDesc),
                                                              _GP, _CP, ctypes.c_double, _VP, _VP]),
    "mugiq_hip_coarse_apply_grid": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.POINTER(CoarseDesc), ctypes.c_int, ctypes.POINTER(CoarseOperatorDesc),
                                                   ctypes.POINTER(CoarseHaloDesc), ctypes.c_int, ctypes.c_double, _VP, _VP]),
    "mugiq_hip_compute_evals_coarse_operator_grid": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.c_int, ctypes.POINTER(CoarseOperatorDesc),
                                                                    ctypes.POINTER(CoarseHaloDesc), ctypes.c_int, ctypes.c_int,
                                                                    ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                                    ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    "mugiq_hip_compute_coarse_operator_coarse": (ctypes.c_int, [ctypes.POINTER(CoarseOperatorDesc), ctypes.POINTER(TransferDesc),
                                                                ctypes.POINTER(CoarseOperatorDesc), _VP, _VP]),
    "mugiq_hip_transfer_set_coarse_vectors": (ctypes.c_int, [ctypes.POINTER(TransferDesc), ctypes.POINTER(CoarseDesc), ctypes.c_int, _VP]),
    "mugiq_hip_transfer_get_coarse_vector": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.POINTER(TransferDesc), ctypes.c_int, _VP]),
    "mugiq_hip_wilson_clover_solve": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, _SP, ctypes.POINTER(ctypes.c_double),
                                                     ctypes.c_int, ctypes.c_double, ctypes.c_int, _I4, ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    "mugiq_hip_mg_solve_param_default": (ctypes.c_int, [ctypes.POINTER(MgSolveParam)]),
    "mugiq_hip_mg_precondition": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                                 ctypes.POINTER(CoarseOperatorDesc), ctypes.POINTER(MgSolveParam), _VP, _VP]),
    "mugiq_hip_mg_solve": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                          ctypes.POINTER(CoarseOperatorDesc), ctypes.POINTER(MgSolveParam), _I4, ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(ctypes.c_double), ctypes.c_int, _I4, _VP, _VP]),
    "mugiq_hip_mg_precondition_grid": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                                      ctypes.POINTER(CoarseOperatorDesc), ctypes.POINTER(CoarseHaloDesc), ctypes.POINTER(MgSolveParam),
                                                      _VP, _VP]),
    "mugiq_hip_mg_solve_grid": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                               ctypes.POINTER(CoarseOperatorDesc), ctypes.POINTER(CoarseHaloDesc), ctypes.POINTER(MgSolveParam), _I4,
                                               ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_int, _I4,
                                               ctypes.POINTER(MgSolveGridInfo), _VP, _VP]),
    "mugiq_hip_mg_rank_sum_plan": (ctypes.c_int, [_I4, _I4, ctypes.c_int, _I4, _I4, _I4, _I4]),
    "mugiq_hip_mg_precondition_sloppy": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                                        ctypes.POINTER(CoarseOperatorDesc), ctypes.POINTER(MgSolveParam), _VP, _VP]),
    "mugiq_hip_mg_solve_mixed": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, _GP, _CP, ctypes.POINTER(TransferDesc),
                                                ctypes.POINTER(CoarseOperatorDesc), ctypes.POINTER(MgSolveParam), _I4, ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(ctypes.c_double), ctypes.c_int, _I4, _VP, _VP]),
    "mugiq_hip_mg_precondition_levels": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                                        ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int, ctypes.POINTER(MgSolveParam), _VP, _VP]),
    "mugiq_hip_mg_solve_levels": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                                 ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int, ctypes.POINTER(MgSolveParam), _I4,
                                                 ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_int, _I4, _VP, _VP]),
    "mugiq_hip_mg_precondition_sloppy_levels": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                                               ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int, ctypes.POINTER(MgSolveParam), _VP, _VP]),
    "mugiq_hip_mg_solve_mixed_levels": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, _GP, _CP, ctypes.POINTER(TransferDesc),
                                                       ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int, ctypes.POINTER(MgSolveParam), _I4,
                                                       ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_int, _I4, _VP, _VP]),
    "mugiq_hip_coarse_deflation_build": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(CoarseDesc), ctypes.c_int,
                                                        ctypes.POINTER(CoarseOperatorDesc), _VP, _VP]),
    "mugiq_hip_coarse_deflate": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.POINTER(CoarseDesc), ctypes.POINTER(CoarseDesc), ctypes.c_int,
                                                ctypes.POINTER(CoarseDeflationDesc), _VP, _VP]),
    "mugiq_hip_mg_precondition_levels_deflated": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                                                 ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int, ctypes.POINTER(MgSolveParam),
                                                                 ctypes.POINTER(CoarseDeflationDesc), _VP, _VP]),
    "mugiq_hip_mg_solve_levels_deflated": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                                          ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int, ctypes.POINTER(MgSolveParam),
                                                          ctypes.POINTER(CoarseDeflationDesc), _I4, ctypes.POINTER(ctypes.c_double),
                                                          ctypes.POINTER(ctypes.c_double), ctypes.c_int, _I4, _VP, _VP]),
    "mugiq_hip_mg_precondition_sloppy_levels_deflated": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, ctypes.POINTER(TransferDesc),
                                                                        ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int, ctypes.POINTER(MgSolveParam),
                                                                        ctypes.POINTER(CoarseDeflationDesc), _VP, _VP]),
    "mugiq_hip_mg_solve_mixed_levels_deflated": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _GP, _CP, ctypes.c_double, _GP, _CP, ctypes.POINTER(TransferDesc),
                                                                ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int, ctypes.POINTER(MgSolveParam),
                                                                ctypes.POINTER(CoarseDeflationDesc), _I4, ctypes.POINTER(ctypes.c_double),
                                                                ctypes.POINTER(ctypes.c_double), ctypes.c_int, _I4, _VP, _VP]),
    "mugiq_hip_mg_convert_precision": (ctypes.c_int, [_SP, _SP, ctypes.c_int, _VP]),
    "mugiq_hip_transfer_convert": (ctypes.c_int, [ctypes.POINTER(TransferDesc), ctypes.POINTER(TransferDesc), _VP]),
    "mugiq_hip_block_orthonormalize": (ctypes.c_int, [ctypes.POINTER(TransferDesc), ctypes.c_int, ctypes.c_double, ctypes.POINTER(BlockOrthoInfo), _VP]),
    "mugiq_hip_transfer_orthonormality": (ctypes.c_int, [ctypes.POINTER(TransferDesc), ctypes.POINTER(ctypes.c_double), _VP]),
    "mugiq_hip_transfer_set_vectors": (ctypes.c_int, [ctypes.POINTER(TransferDesc), _SP, ctypes.c_int, _VP]),
    "mugiq_hip_transfer_get_vector": (ctypes.c_int, [_SP, ctypes.POINTER(TransferDesc), ctypes.c_int, _VP]),
    "mugiq_hip_mg_setup_param_default": (ctypes.c_int, [ctypes.POINTER(MgSetupParam)]),
    "mugiq_hip_mg_setup": (ctypes.c_int, [ctypes.POINTER(TransferDesc), ctypes.POINTER(CoarseOperatorDesc), _SP, ctypes.c_int, _GP, _CP, ctypes.c_double,
                                          ctypes.POINTER(MgSetupParam), ctypes.POINTER(MgSetupInfo), _VP, _VP]),
    "mugiq_hip_coarse_gram": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(CoarseDesc), ctypes.c_int, ctypes.POINTER(CoarseDesc),
                                             ctypes.c_int, _VP, _VP]),
    "mugiq_hip_coarse_rotate": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.c_int, ctypes.POINTER(CoarseDesc), ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    "mugiq_hip_hermitian_eigh": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(ctypes.c_double)]),
    "mugiq_hip_cholesky_upper": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_double, _I4,
                                                ctypes.POINTER(ctypes.c_double)]),
    "mugiq_hip_upper_triangular_inverse": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "mugiq_hip_coarse_eig_param_default": (ctypes.c_int, [ctypes.POINTER(CoarseEigParam)]),
    "mugiq_hip_coarse_eigensolve": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.POINTER(CoarseDesc), ctypes.POINTER(CoarseOperatorDesc), ctypes.c_int,
                                                   ctypes.POINTER(CoarseEigParam), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                   ctypes.POINTER(ctypes.c_double), ctypes.POINTER(CoarseEigInfo), _VP, _VP]),
    "mugiq_hip_coarse_gram_grid": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(CoarseDesc), ctypes.c_int, ctypes.POINTER(CoarseDesc),
                                                  ctypes.c_int, _VP, _VP]),
    "mugiq_hip_coarse_eigensolve_grid": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.POINTER(CoarseDesc), ctypes.POINTER(CoarseOperatorDesc),
                                                        ctypes.POINTER(CoarseHaloDesc), ctypes.c_int, ctypes.POINTER(CoarseEigParam),
                                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                        ctypes.POINTER(CoarseEigInfo), ctypes.POINTER(CoarseEigGridInfo), _VP, _VP]),
    "mugiq_hip_prolongate_batched": (ctypes.c_int, [_SP, ctypes.POINTER(CoarseDesc), ctypes.c_int, ctypes.POINTER(TransferDesc), _VP]),
    "mugiq_hip_prolongate_contract_batched": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.POINTER(CoarseDesc), ctypes.POINTER(ctypes.c_double),
                                                             ctypes.c_int, ctypes.POINTER(TransferDesc), _VP]),
    "mugiq_hip_restrict_batched": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), _SP, ctypes.c_int, ctypes.POINTER(TransferDesc), ctypes.c_int, _VP]),
    "mugiq_hip_restrict_coarse_batched": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.POINTER(CoarseDesc), ctypes.c_int,
                                                         ctypes.POINTER(TransferDesc), _VP]),
    "mugiq_hip_transfer_form": (ctypes.c_int, [ctypes.POINTER(TransferDesc), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.POINTER(TransferForm)]),
    "mugiq_hip_deflate_low_modes_coarse": (ctypes.c_int, [_SP, _SP, ctypes.c_int, ctypes.POINTER(CoarseDesc), ctypes.POINTER(ctypes.c_double),
                                                          ctypes.c_int, ctypes.POINTER(TransferDesc), ctypes.c_int, ctypes.c_int,
                                                          ctypes.POINTER(ctypes.c_double), _VP, _VP]),
    # driver (struct pointers are passed with ctypes.byref; see mugiq_amd/loop.py for the struct definitions)
    "mugiq_hip_loop_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _VP, _SP, ctypes.POINTER(ctypes.c_double),
                                             ctypes.c_int, _VP, _VP]),
    "mugiq_hip_loop_create_coarse_levels": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _VP, ctypes.POINTER(CoarseDesc),
                                                           ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(TransferDesc),
                                                           ctypes.c_int, ctypes.c_int, _VP, _VP]),
    "mugiq_hip_prolongate_coarse_batched": (ctypes.c_int, [ctypes.POINTER(CoarseDesc), ctypes.POINTER(CoarseDesc), ctypes.c_int,
                                                           ctypes.POINTER(TransferDesc), _VP]),
    "mugiq_hip_loop_create_coarse": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _VP, ctypes.POINTER(CoarseDesc),
                                                    ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(TransferDesc),
                                                    ctypes.c_int, _VP, _VP]),
    "mugiq_hip_loop_create_two_sided": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _VP, _SP, _SP, ctypes.POINTER(ctypes.c_double),
                                                       ctypes.c_int, _VP, _VP]),
    "mugiq_hip_loop_compute": (ctypes.c_int, [_VP]),
    "mugiq_hip_fused_form": (ctypes.c_int, [_SP, ctypes.c_int, ctypes.c_int, _I4, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(FusedForm)]),
    "mugiq_hip_loop_plan": (ctypes.c_int, [_VP, _SP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _I4, ctypes.c_size_t, ctypes.POINTER(LoopPlan)]),
    "mugiq_hip_loop_deflate": (ctypes.c_int, [_VP, _SP, _SP, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "mugiq_hip_loop_deflate_coarse": (ctypes.c_int, [_VP, _SP, _SP, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "mugiq_hip_loop_get_info": (ctypes.c_int, [_VP, _VP]),
    "mugiq_hip_loop_set_profiling": (ctypes.c_int, [_VP, ctypes.c_int]),
    "mugiq_hip_loop_get_phases": (ctypes.c_int, [_VP, _VP, ctypes.c_int]),
    "mugiq_hip_loop_get_entry": (ctypes.c_int, [_VP, ctypes.c_int, _I4]),
    "mugiq_hip_loop_entry_derived_from": (ctypes.c_int, [_VP, ctypes.c_int]),
    "mugiq_hip_loop_get_entry_kernel": (ctypes.c_int, [_VP, ctypes.c_int]),
    "mugiq_hip_loop_ultra_local_carrier": (ctypes.c_int, [_VP]),
    "mugiq_hip_loop_halos_packed_in_entry": (ctypes.c_int, [_VP]),
    "mugiq_hip_loop_data_pos_d": (_VP, [_VP]),
    "mugiq_hip_loop_data_pos_h": (_VP, [_VP]),
    "mugiq_hip_loop_data_mom_bcast_h": (_VP, [_VP]),
    "mugiq_hip_loop_write_hdf5": (ctypes.c_int, [_VP]),
    "mugiq_hip_write_loops_hdf5_mom": (ctypes.c_int, [ctypes.c_char_p, _VP, ctypes.c_int, ctypes.c_int, _I4, ctypes.c_int,
                                                      ctypes.POINTER(ctypes.c_char_p), _I4, _I4, ctypes.c_int, ctypes.c_int]),
    "mugiq_hip_loop_destroy": (ctypes.c_int, [_VP]),
    "mugiq_hip_extended_gauge_bytes": (ctypes.c_size_t, [_I4, _I4, ctypes.c_int]),
    "mugiq_hip_alloc_extended_gauge": (ctypes.c_int, [_GP, _I4, _I4, ctypes.c_int]),
    "mugiq_hip_free_extended_gauge": (ctypes.c_int, [_GP]),
    "mugiq_hip_create_extended_gauge": (ctypes.c_int, [_GP, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, _VP, _VP]),
    "mugiq_hip_parse_displace_entry_string": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, _I4, _I4]),
    "mugiq_hip_parse_displacement": (ctypes.c_int, [ctypes.c_char_p, _I4, _I4]),
}

_lib = None


def load():
    """Load the library once; raise (never fall back) if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not found: build it with `make -C mugiq_amd/csrc` or "
                          "`python -c 'import __graft_entry__ as g; g.build()'` -- there is no CPU fallback" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status):
    if status != 0:
        msg = load().mugiq_hip_last_error()
        raise MugiqHipError("status %d: %s" % (status, msg.decode() if msg else "?"))


def int4(v):
    return (ctypes.c_int * 4)(*[int(x) for x in v])
