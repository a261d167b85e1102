"""mugiq_amd -- MI355X-native (HIP / gfx950) drop-in for the disconnected-loop hot path of ckallidonis/mugiq.

The product is libmugiq_hip.so (C ABI in include/mugiq_hip.h).  This package is the Python host-side mirror
of MuGiq's operator interface over that ABI; importing it loads the library and fails loudly if it is missing.
"""
from . import _lib

_lib.load()

from .fields import SpinorField, GaugeField, CloverField, CoarseField, CoarseOperator, CoarseHalo, Transfer, FLOAT2, FLOAT4  # noqa: E402
from .operators import (  # noqa: E402
    copyGammaCoeffStructToSymbol, copyGammaMapStructToSymbol, gammaTables, GammaName,
    performLoopContraction, performLoopContractionBatched, performCovariantDisplacementVector, packFace, exchangeGhostVec,
    createPhaseMatrixGPU, convertIdxOrder_mapGamma, momentumProjection, momentumProjectionSeparable, convertAndProject, convertAndProjectSlots, convertAndProjectPlan, packFaceLayers, displacedLoopContractionFused, displacedLoopContractionFusedTwoSided, reflectDisplacedLoop, packLoopLayers, probeReadBandwidth, prolongateEvecs, prolongateCoarseEvecs, prolongateContractBatched,
    deflateLowModes, restrictVecs, restrictCoarseVecs, deflateLowModesCoarse, transferForm,
    PROLONG_FAMILY_MFMA, PROLONG_FAMILY_VECTOR_STAGED, PROLONG_FAMILY_VECTOR_GLOBAL,
    CONTRACT_FAMILY_COARSE_MFMA, CONTRACT_FAMILY_COARSE_VECTOR, CONTRACT_FAMILY_DIRECT_STAGED, CONTRACT_FAMILY_DIRECT_GLOBAL,
    DispDir, DispSignMinus, DispSignPlus, LOOP_FT_SIGN_MINUS, LOOP_FT_SIGN_PLUS, DisplaceFlagArray,
    REGION_ALL, REGION_INTERIOR, REGION_BOUNDARY, REGION_OVERWRITE, ENTRY_KERNEL_REFLECTED, ENTRY_KERNEL_MFMA_COLUMN, ENTRY_KERNEL_MFMA_ROW,
    ENTRY_KERNEL_VECTOR_TILE, ENTRY_KERNEL_STREAMING, ENTRY_KERNEL_STEPWISE,
    PROJECT_FORM_GENERAL, PROJECT_FORM_PIPELINED, PROJECT_FORM_MFMA,
)
from ._lib import MugiqHipError, LIB_PATH  # noqa: E402
from .loop import (  # noqa: E402
    MugiqLoopParam, Loop_Mugiq, loopPlan, fusedForm, parseDisplaceEntryString, parseDisplacement, read_momenta_file, writeLoopsHDF5_Mom, reflectMomentumSpace,
    LOOP_CALC_TYPE_BLAS, LOOP_CALC_TYPE_OPT_KERNEL, LOOP_CALC_TYPE_BASIC_KERNEL,
    FUSED_FAMILY_NONE, FUSED_FAMILY_MFMA_COLUMN, FUSED_FAMILY_MFMA_ROW, FUSED_FAMILY_TILE32, FUSED_FAMILY_TILE16, FUSED_FAMILY_STREAMING,
)
from .comm import GridComm, RcclComm  # noqa: E402
from .displace import Displace, DISPLACE_TYPE_COVARIANT  # noqa: E402
from .eigsolve import (  # noqa: E402
    Eigsolve_Mugiq, wilsonApply, computeEvals, computeEvalsCoarse, computeCoarseOperator, computeCoarseOperatorCoarse, coarseApply, coarseApplyForm, computeCoarseOperatorGrid, coarseApplyGrid, computeEvalsCoarseGrid, projectVector, wilsonSolve, SolveInfo,
    mgSolve, mgPrecondition, mgSolveMixed, mgPreconditionSloppy, mgConvertPrecision, mgSolveParam, MgSolveInfo, mgSetup, mgSetupCoarse, MgSetupCoarseInfo, mgSetupParam, mgStartVectors, MgSetupInfo,
    coarseGram, coarseRotate, hermitianEigh, choleskyUpper, upperTriangularInverse, coarseEigensolve, coarseEigParam, coarseStartVectors, CoarseEigInfo,
    coarseGramGrid, coarseStartVectorsGrid, coarseEigensolveGrid, CoarseEigGridInfo,
    mgPreconditionGrid, mgSolveGrid, mgRankSumPlan, MgSolveGridInfo,
    CoarseDeflation, coarseDeflate,
    MUGIQ_EIG_OPERATOR_M, MUGIQ_EIG_OPERATOR_Mdag, MUGIQ_EIG_OPERATOR_MdagM, MUGIQ_EIG_OPERATOR_MMdag, MUGIQ_EIG_OPERATOR_H,
)

__all__ = [n for n in dir() if not n.startswith("_")]
