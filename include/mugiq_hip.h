/*
 * mugiq_hip.h -- C ABI of libmugiq_hip.so, the MI355X-native (HIP / gfx950) drop-in for the
 * disconnected-loop hot path of ckallidonis/mugiq.
 *
 * Every entry point names the reference interface it replaces (file:line, relative to the MuGiq tree).
 * The reference's operator API is a set of C++ templates over QUDA types
 * (lib/contract_wrappers.cu, declared at include/loop_mugiq.h:280-311 and include/displace.h:109-111);
 * QUDA types cannot cross a C ABI, so each function takes plain pointers plus the POD descriptors below,
 * which carry exactly what the reference's Arg structs read out of a ColorSpinorField / cudaGaugeField
 * (include/contract_util.cuh:69-194).  include/mugiq_hip_operators.hpp re-declares the reference's
 * template names on top of this ABI; INTEGRATION.md shows the QUDA-side adapter.
 *
 * Conventions
 *  - all data pointers are DEVICE pointers unless the parameter name ends in _h;
 *  - every function returns 0 on success and a non-zero MugiqHipStatus on failure; the message is
 *    available from mugiq_hip_last_error() (the reference aborts through errorQuda instead:
 *    lib/contract_wrappers.cu:100,138,185);
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls are asynchronous on
 *    that stream; nothing in this library calls hipDeviceSynchronize on the data path;
 *  - the caller owns every buffer.  Loop buffers are ACCUMULATED into (+=) and must be zeroed by the
 *    caller, as in the reference (lib/loop_mugiq.cpp:138,476).
 */
#ifndef MUGIQ_HIP_H
#define MUGIQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUGIQ_HIP_VERSION 100

typedef enum MugiqHipStatus_e {
  MUGIQ_HIP_SUCCESS = 0,
  MUGIQ_HIP_ERROR_INVALID_ARGUMENT = 1, /* precondition the reference checks with errorQuda */
  MUGIQ_HIP_ERROR_UNSUPPORTED = 2,
  MUGIQ_HIP_ERROR_HIP = 3,              /* a HIP runtime call failed (reference: checkCudaError) */
  MUGIQ_HIP_ERROR_NO_DEVICE = 4,
  MUGIQ_HIP_ERROR_NOT_CONVERGED = 5     /* mugiq_hip_wilson_solve: maxIter reached; the outputs are filled all the same */
} MugiqHipStatus;

/* Values are those of QudaPrecision / QudaFieldOrder so an adapter can pass them through. */
#define MUGIQ_HIP_SINGLE_PRECISION 4
#define MUGIQ_HIP_DOUBLE_PRECISION 8
#define MUGIQ_HIP_FLOAT2_FIELD_ORDER 2
#define MUGIQ_HIP_FLOAT4_FIELD_ORDER 4

/* include/enum_mugiq.h:72-85 */
#define MUGIQ_HIP_DISP_DIR_X 0
#define MUGIQ_HIP_DISP_DIR_Y 1
#define MUGIQ_HIP_DISP_DIR_Z 2
#define MUGIQ_HIP_DISP_DIR_T 3
#define MUGIQ_HIP_DISP_SIGN_MINUS 0
#define MUGIQ_HIP_DISP_SIGN_PLUS 1

/*
 * A nSpin=4, nColor=3 colour-spinor field in QUDA's native even-odd layout: what
 * colorspinor::FieldOrderCB<Float,4,3,1,order> (include/contract_util.cuh:20-21) addresses.
 * Complex-element index of component k = 3*spin + colour at (parity, x_cb):
 *   FLOAT2: parity*parity_offset + k*stride + x_cb
 *   FLOAT4: parity*parity_offset + ((k/2)*stride + x_cb)*2 + (k%2)
 * ghost[dim][0|1] are the backward / forward ghost zones filled by a halo exchange of depth 1
 * (reference: ColorSpinorField::exchangeGhost, lib/contract_wrappers.cu:166-169); each zone is itself
 * laid out like a field body with volumeCB = stride = faceCB(dim), parity_offset = 12*faceCB(dim),
 * indexed by QUDA's ghostFaceIndex.  They are read only for partitioned dims (commDim[dim] != 0).
 */
typedef struct MugiqHipSpinorField_s {
  void *data;            /* ColorSpinorField::V() */
  int precision;         /* 4 | 8 */
  int field_order;       /* 2 | 4 */
  int nParity;           /* SiteSubset(); the hot path requires 2 (lib/contract_wrappers.cu:100,185) */
  int volumeCB;          /* VolumeCB() */
  int stride;            /* Stride() = volumeCB + pad */
  int X[4];              /* full local lattice dims (x,y,z,t), all even */
  int64_t parity_offset; /* complex elements between the two parities = Bytes()/2/sizeof(complex) */
  void *ghost[4][2];     /* may be all NULL on a single domain */
} MugiqHipSpinorField;

/*
 * The border-extended gauge field Displace builds (lib/displace.cpp:104-134), in QUDA's native
 * FLOAT2 gauge order with 18 reals per link (gauge_mapper<Float,QUDA_RECONSTRUCT_NO>,
 * include/contract_util.cuh:23-24): complex index of element (row,col) of link (dir, x_cb, parity)
 *   parity*parity_offset + (dir*9 + row*3 + col)*stride + x_cb
 * with x_cb the even-odd index on the EXTENDED lattice dimEx = X + 2*R.
 */
typedef struct MugiqHipGaugeField_s {
  void *data;
  int precision;         /* 4 | 8 */
  int X[4];              /* interior (non-extended) local dims */
  int R[4];              /* border per dim; reference uses 2*commDimPartitioned (lib/displace.cpp:16) */
  int stride;            /* extended volumeCB + pad */
  int64_t parity_offset; /* complex elements between parities */
} MugiqHipGaugeField;

/* ---- housekeeping ------------------------------------------------------------------------------- */
int mugiq_hip_version(void);
const char *mugiq_hip_last_error(void);
/* number of visible HIP devices (0 if none); does not initialise a context */
int mugiq_hip_device_count(void);
/* Streams and re-entrancy.  Every entry point that launches kernels takes the HIP stream they run on.  The small device
 * tables a call uploads for its kernels (eigenvector pointer lists, 1/sigma, momenta) and the workspaces the library
 * allocates when the caller passes none are kept PER (device, stream): calls issued on different streams -- from one
 * thread or several, through free operators or through different MugiqHipLoop objects -- are independent; calls on
 * one stream are ordered by the stream.  (The reference's wrappers are single-stream and not re-entrant: per-call
 * cudaMalloc + cudaDeviceSynchronize, lib/contract_wrappers.cu:93-114.)  Two host threads must not issue calls on the
 * SAME stream at the same time.  mugiq_hip_release_stream drains `stream` and frees what the library holds for it; call
 * it before destroying a stream that was passed to this library (optional: the buffers are small and are reused if the
 * handle value comes back). */
int mugiq_hip_release_stream(void *stream);

/* Roofline calibration (measurement aid, not part of the reference): stream-read `bytes` of buf_d once with 16-B
 * loads per lane (plain or non-temporal) and write nothing.  Time it with events to get the achievable HBM read
 * bandwidth of the device at hand. */
int mugiq_hip_probe_read_bandwidth(const void *buf_d, size_t bytes, int nonTemporal, void *stream);

/* Test aid (not part of the reference): overwrite the LDS of every CU with NaN bit patterns.  LDS is not cleared between kernels;
 * a kernel that reads a cell it never wrote computes with whatever the previous kernel left there, which is usually finite.  With
 * this call in front such a read shows up in the result (tests/test_gpu_driver.py::test_kernels_do_not_read_unwritten_lds). */
int mugiq_hip_debug_poison_lds(void *stream);

/* ---- gamma tables ------------------------------------------------------------------------------- */
/* copyGammaCoeffStructToSymbol<Float>()  lib/contract_wrappers.cu:6-19
 * copyGammaMapStructToSymbol<Float>()    lib/contract_wrappers.cu:26-43
 * The tables are compile-time constants of the HIP kernels, so these only validate `precision`;
 * they are kept so Loop_Mugiq::copyGammaToConstMem (lib/loop_mugiq.cpp:162-167) maps 1:1. */
int mugiq_hip_copy_gamma_coeff_to_symbol(int precision);
int mugiq_hip_copy_gamma_map_to_symbol(int precision);
/* Host copies of the tables the kernels were compiled with (include/gamma.h:32-71,99-109):
 * row_value[16][4][2] (re,im), column_index[16][4], map_sign[16], map_index[16]. Any pointer may be NULL. */
int mugiq_hip_get_gamma_tables(double *row_value_h, int *column_index_h, double *map_sign_h, int *map_index_h);
/* GammaName(m)  include/gamma.h:11-20 ; NULL if m is out of range */
const char *mugiq_hip_gamma_name(int m);

/* ---- a1/a2  ultra-local or displaced loop contraction ------------------------------------------------ */
/* performLoopContraction<Float,order>(loopData_d, eVecL, eVecR, sigma)   lib/contract_wrappers.cu:88-115
 * kernel loopContract_kernel lib/mugiq_contract_kernels.cu:45-122:
 *   loopData[tid + V*iG] += (1/sigma) * vL^dag(x) G(iG) vR(x),  tid = x_cb + parity*volumeCB, iG in [0,16)
 * loopData_d: complex<Float>[16*V] of the fields' precision. */
int mugiq_hip_perform_loop_contraction(void *loopData_d, const MugiqHipSpinorField *eVecL,
                                       const MugiqHipSpinorField *eVecR, double sigma, void *stream);

/* The fast path (new): the eigenvector loop of Loop_Mugiq::computeCoarseLoop (lib/loop_mugiq.cpp:478-503)
 * folded into one launch: loopData += sum_{n<nVec} (1/sigma[n]) vL_n^dag G vR_n with the 16 accumulators
 * held in registers, so each eigenvector is read once and loopData is touched once.
 * eVecL_h/eVecR_h: host arrays of nVec descriptors (same geometry, precision, order); sigma_h: host doubles
 * (eVals_sigma, cast to Float as at lib/loop_mugiq.cpp:479).  eVecR_h may equal eVecL_h (ultra-local). */
int mugiq_hip_perform_loop_contraction_batched(void *loopData_d, const MugiqHipSpinorField *eVecL_h,
                                               const MugiqHipSpinorField *eVecR_h, const double *sigma_h,
                                               int nVec, void *stream);

/* Mixed precision (BASELINE.json configs[3]; beyond the reference, which is single-typed end to end): loopPrecision = 8
 * with fp32 eigenvectors keeps the storage in fp32 and does all arithmetic, the 16-gamma accumulation over the
 * eigenvectors and the loop buffer in fp64.  loopPrecision = 0 or = the fields' precision is the plain call. */
int mugiq_hip_perform_loop_contraction_batched_mixed(void *loopData_d, int loopPrecision,
                                                     const MugiqHipSpinorField *eVecL_h,
                                                     const MugiqHipSpinorField *eVecR_h, const double *sigma_h,
                                                     int nVec, void *stream);

/* ---- a4/a5  covariant displacement --------------------------------------------------------------------- */
/* performCovariantDisplacementVector<Float,order>(dst, src, gauge, dispDir, dispSign)
 * lib/contract_wrappers.cu:171-198, kernel lib/mugiq_displace_kernels.cu:156-185:
 *   dst(x) = U_d(x) src(x+d)  (sign +)   |   dst(x) = U_d^dag(x-d) src(x-d)  (sign -)
 * commDim[4] replaces QUDA's global comm_dim_partitioned() (include/contract_util.cuh:89): for a
 * partitioned dim the neighbour of an on-face site is read from src->ghost[dim][bnd].  The halo
 * exchange itself (exchangeGhostVec, :166-169) is the caller's job -- see mugiq_hip_pack_face. */
int mugiq_hip_perform_covariant_displacement_vector(const MugiqHipSpinorField *dst,
                                                    const MugiqHipSpinorField *src,
                                                    const MugiqHipGaugeField *gauge, int dispDir,
                                                    int dispSign, const int commDim[4], void *stream);

/* Pack the face of `src` a neighbour needs as its depth-1 ghost zone, in ghostFaceIndex order
 * (the send half of ColorSpinorField::exchangeGhost, lib/contract_wrappers.cu:166-169).
 *   high = 0: low face  (x[dim] = 0)        -> the backward neighbour's ghost[dim][1]
 *   high = 1: high face (x[dim] = X[dim]-1) -> the forward  neighbour's ghost[dim][0]
 * face_d: 2*12*faceCB complex elements of the field's precision, laid out as a ghost zone. */
int mugiq_hip_pack_face(void *face_d, const MugiqHipSpinorField *src, int dim, int high, void *stream);

/* Batched, multi-layer version for the fused path: for every eigenvector n < nVec and layer j < layers pack the
 * face x[dim] = j (high = 0) or x[dim] = X[dim]-1-j (high = 1) into
 * faces_d[n][j] = one ghost zone (2*12*faceCB complex), contiguous over (n, j) so one message carries them all. */
int mugiq_hip_pack_face_layers(void *faces_d, const MugiqHipSpinorField *eVecs_h, int nVec, int dim, int high,
                               int layers, void *stream);

/* ---- reflected displacement entries (new) ----------------------------------------------------------------------
 * The reference computes the "+mu" and "-mu" entries of a displacement independently (lib/loop_mugiq.cpp:478-500).
 * Because W_{-k}(x) = W_{+k}(x - k mu)^dagger, gamma matrices commute with colour matrices and sigma_n is real,
 *     L^-_{k,G}(x) = eta_G conj( L^+_{k,G}(x - k mu) ),   L^+_{k,G}(x) = eta_G conj( L^-_{k,G}(x + k mu) ),
 * eta_G = +-1 with G^dagger = eta_G G.  dstSlot_d / srcSlot_d: one loop slot each (16*V complex of `precision`, the
 * dataPos layout loopData[tid + V*iG]); dstDispSign = sign of the entry being derived; length = k.  If
 * commDim[dispDir] != 0, ghostLayers_d holds the k boundary layers of the neighbour's source slot as
 * mugiq_hip_pack_loop_layers writes them (dst "-": the backward neighbour's HIGH layers; dst "+": the forward
 * neighbour's LOW layers). */
int mugiq_hip_reflect_displaced_loop(void *dstSlot_d, const void *srcSlot_d, const void *ghostLayers_d, const int localL[4],
                                     int dispDir, int dstDispSign, int length, const int commDim[4], int precision,
                                     void *stream);

/* layers_d[((j*16 + iG)*2 + parity)*faceCB + ghostFaceIndex] = slot value at x[dim] = X[dim]-layers+j (high = 1) or
 * x[dim] = j (high = 0), j < layers: 32*layers*faceCB complex of `precision`. */
int mugiq_hip_pack_loop_layers(void *layers_d, const void *slot_d, const int localL[4], int dim, int high, int layers,
                               int precision, void *stream);

/* ---- fused displaced contraction (new; the fast form of lib/loop_mugiq.cpp:485-497) --------------------------- */
/* For one displacement entry (dispDir, dispSign) and the lengths kValues_h[0..nK):
 *   loopData_d[slot i][tid + V*iG] += sum_n (1/sigma_n) v_n^dag(x) G(iG) W_k(x) v_n(x +- k mu),  k = kValues_h[i]
 * where W_k is the path-ordered link product, handed over as pathLinkFields_h[i] = device pointer to the field
 * E_k = D^k E_0, E_0(x)(s,c) = delta_sc for s < 3 (a FLOAT2 spinor field with stride = volumeCB, pad 0, of the
 * eigenvectors' precision) -- i.e. the output of k applications of
 * mugiq_hip_perform_covariant_displacement_vector to E_0.  The displaced vectors are never materialised.
 * Slots are 16*V complex apart.  If commDim[dispDir] != 0, ghostLayers_d holds `layers` >= max k face layers
 * of every eigenvector received from the neighbour the displacement points to, laid out as
 * mugiq_hip_pack_face_layers writes them (sign +: the forward neighbour's LOW layers; sign -: the backward
 * neighbour's HIGH layers).
 * Links need not be unitary: the result is that of the links as stored.  The matrix-pipe tile (the default kernel) is exact only
 * where the axial gauge built from W_1 .. W_kmax is, g^dag g = 1; these calls build that gauge, reduce
 * max |g^dag g - 1| over it and take the tile only below 1e-12 (fp64 storage) / 4e-6 (fp32), else the vector tiles.  The check reads
 * the deviation back to the host: a call that may take the tile synchronises `stream` once. */
int mugiq_hip_displaced_loop_contraction_fused(void *loopData_d, const MugiqHipSpinorField *eVecs_h,
                                               const double *sigma_h, int nVec, const void *const *pathLinkFields_h,
                                               const int *kValues_h, int nK, int dispDir, int dispSign,
                                               const int commDim[4], const void *ghostLayers_d, int layers,
                                               void *stream);

int mugiq_hip_displaced_loop_contraction_fused_mixed(void *loopData_d, int loopPrecision,
                                                     const MugiqHipSpinorField *eVecs_h, const double *sigma_h, int nVec,
                                                     const void *const *pathLinkFields_h, const int *kValues_h, int nK,
                                                     int dispDir, int dispSign, const int commDim[4],
                                                     const void *ghostLayers_d, int layers, void *stream);

/* The same restricted to a region, so the halo transfer can overlap the part that does not need it:
 *   MUGIQ_HIP_REGION_INTERIOR: sites whose shifted reads x +- k mu stay inside the local lattice (ghostLayers_d not read,
 *                              may still be in flight);   MUGIQ_HIP_REGION_BOUNDARY: the remaining sites;
 *   INTERIOR followed by BOUNDARY on the same loop slots == MUGIQ_HIP_REGION_ALL. */
#define MUGIQ_HIP_REGION_ALL 0
#define MUGIQ_HIP_REGION_INTERIOR 1
#define MUGIQ_HIP_REGION_BOUNDARY 2
/* OR-ed into `region`: the addressed sites of the slots are WRITTEN instead of accumulated into -- the caller vouches that
 * they hold nothing yet and saves the memset of the slots and the read half of the read-modify-write. */
#define MUGIQ_HIP_REGION_OVERWRITE 0x100
int mugiq_hip_displaced_loop_contraction_fused_region(void *loopData_d, int loopPrecision,
                                                      const MugiqHipSpinorField *eVecs_h, const double *sigma_h, int nVec,
                                                      const void *const *pathLinkFields_h, const int *kValues_h, int nK,
                                                      int dispDir, int dispSign, const int commDim[4],
                                                      const void *ghostLayers_d, int layers, int region, void *stream);
/* The same, and in the same pass over the eigenvectors the ULTRA-LOCAL loop (displacement 0: the loop of lib/loop_mugiq.cpp:499-503,
 * sum_n (1/sigma_n) v_n^dag G v_n) into ultraLocalSlot_d (16*V complex, same region / overwrite semantics as the displaced slots):
 * it rides along as one more slot (k = 0, W = 1) of the tiled kernel when that has room -- a free slot of its 12-wave forms, or
 * the fourth slot of the 16-wave form (fp64 FLOAT2 column tiles with three lengths) -- which saves the separate pass over all
 * eigenvectors.  *carried = 1 if the slot was produced, 0 if not (then nothing was written to it and the caller computes it
 * with mugiq_hip_perform_loop_contraction_batched).  The slot is produced for the whole lattice or not at all: with a
 * region other than MUGIQ_HIP_REGION_ALL it is never taken along (*carried = 0).  ultraLocalSlot_d = NULL: plain _region call. */
int mugiq_hip_displaced_loop_contraction_fused_carry(void *loopData_d, int loopPrecision,
                                                     const MugiqHipSpinorField *eVecs_h, const double *sigma_h, int nVec,
                                                     const void *const *pathLinkFields_h, const int *kValues_h, int nK,
                                                     int dispDir, int dispSign, const int commDim[4],
                                                     const void *ghostLayers_d, int layers, int region,
                                                     void *ultraLocalSlot_d, int *carried, void *stream);

/* Two-sided form (new): the same contraction with separate LEFT and RIGHT vector sets,
 *   loopData_d[slot i][tid + V*iG] += sum_n (1/sigma_n) vL_n^dag(x) G(iG) W_k(x) vR_n(x +- k mu),
 * e.g. the deflated stochastic part of a disconnected loop (vL = gamma5 xi_r, vR = phi_r: INTEGRATION.md).  The signature of
 * the _carry call with eVecL_h / eVecR_h in place of eVecs_h (same geometry, precision and order); the ghost layers are those of
 * the RIGHT set (the only one that is displaced), the ultra-local slot is sum_n (1/sigma_n) vL_n^dag G vR_n.  It runs on the
 * matrix-pipe tile (csrc/fused_mfma_kernel.h, two-sided form) only: MUGIQ_HIP_ERROR_UNSUPPORTED where that tile does not take the
 * entry (lengths > 8 or not ascending, a partitioned x axis, no tile geometry for the extent, links whose axial gauge is not unitary
 * to the tolerance of the one-sided calls) -- then the caller displaces vR step
 * by step (mugiq_hip_perform_covariant_displacement_vector) and contracts with mugiq_hip_perform_loop_contraction_batched. */
int mugiq_hip_displaced_loop_contraction_fused_two_sided(void *loopData_d, int loopPrecision,
                                                         const MugiqHipSpinorField *eVecL_h, const MugiqHipSpinorField *eVecR_h,
                                                         const double *sigma_h, int nVec, const void *const *pathLinkFields_h,
                                                         const int *kValues_h, int nK, int dispDir, int dispSign,
                                                         const int commDim[4], const void *ghostLayers_d, int layers, int region,
                                                         void *ultraLocalSlot_d, int *carried, void *stream);

/* ---- a8  Fourier phase matrix -------------------------------------------------------------------------- */
/* createPhaseMatrixGPU<Float>(phaseMatrix_d, momMatrix_h, locV3, Nmom, FTSign, localL, totalL)
 * lib/contract_wrappers.cu:50-77, kernel lib/mugiq_util_kernels.cu:3-35.  commCoord[4] replaces QUDA's
 * comm_coord() (include/contract_util.cuh:64).  momMatrix_h: int[Nmom][3], MOM_MATRIX_IDX(id,im)=id+3*im. */
int mugiq_hip_create_phase_matrix(void *phaseMatrix_d, const int *momMatrix_h, long long locV3, int Nmom,
                                  int FTSign, const int localL[4], const int totalL[4],
                                  const int commCoord[4], int precision, void *stream);

/* ---- a9  even-odd -> time-major reorder with the G -> g5 G map ------------------------------------------ */
/* convertIdxOrder_mapGamma<Float>(dataPosMP_d, dataPos_d, nData, nLoop, nParity, volumeCB, localL)
 * lib/contract_wrappers.cu:133-156, kernel lib/mugiq_util_kernels.cu:59-99 */
int mugiq_hip_convert_idx_order_map_gamma(void *dataPosMP_d, const void *dataPos_d, int nData, int nLoop,
                                          int nParity, int volumeCB, const int localL[4], int precision,
                                          void *stream);

/* ---- a10  momentum projection (the cublasZgemm/Cgemm of lib/loop_mugiq.cpp:363-378) ---------------------- */
/* dataMom_d[M x N] = dataPosMP_d[M x K] * phaseMatrix_d[K x N], column-major, M = locT*nData, K = locV3,
 * N = Nmom, alpha = 1, beta = 0.  workspace_d may be NULL (the library then allocates its own scratch);
 * mugiq_hip_momentum_projection_workspace returns the bytes it would like. */
size_t mugiq_hip_momentum_projection_workspace(int locT, int nData, long long locV3, int Nmom, int precision);
int mugiq_hip_momentum_projection(void *dataMom_d, const void *dataPosMP_d, const void *phaseMatrix_d,
                                  int locT, int nData, long long locV3, int Nmom, int precision,
                                  void *workspace_d, size_t workspace_bytes, void *stream);

/* The same projection without the dense phase matrix (new).  exp(i s 2 pi p.x/L) factorises over x, y, z, so the sum over
 * the local spatial volume is taken one direction at a time, for the distinct p_x, then the distinct (p_x, p_y), then
 * the momenta: A is read once and the work drops from K*Nmom to about K*(number of distinct p_x) complex multiply-adds
 * per row.  Takes what createPhaseMatrixGPU takes (momMatrix_h [Nmom][3], FTSign, localL, totalL, commCoord) instead of
 * its output; the phases are rounded like the reference's, one direction at a time.  Same result to rounding. */
size_t mugiq_hip_momentum_projection_separable_workspace(const int *momMatrix_h, int Nmom, const int localL[4], int locT,
                                                          int nData, int precision);
int mugiq_hip_momentum_projection_separable(void *dataMom_d, const void *dataPosMP_d, const int *momMatrix_h, int Nmom,
                                            int FTSign, const int localL[4], const int totalL[4], const int commCoord[4],
                                            int locT, int nData, int precision, void *workspace_d, size_t workspace_bytes,
                                            void *stream);

/* a9 + a10 in one call (new): dataMom_d[M x Nmom] from the even-odd position-space buffer dataPos_d ([nData][V], the input
 * of convertIdxOrder_mapGamma).  The reorder with the G -> g5 G map and the sum over x happen in one kernel, so the
 * reordered copy dataPosMP is neither written nor read; then the y and z steps of the separable projection.
 * Workspace as for mugiq_hip_momentum_projection_separable. */
int mugiq_hip_convert_and_project(void *dataMom_d, const void *dataPos_d, int nData, int nLoop, const int *momMatrix_h, int Nmom,
                                  int FTSign, const int localL[4], const int totalL[4], const int commCoord[4], int precision,
                                  void *workspace_d, size_t workspace_bytes, void *stream);

/* The same for a SUBSET of the loop slots (new): only the slots slots_h[0 .. nSlots) of dataPos_d ([nLoop][16][V]) are read,
 * and only their rows t + locT*(ig + 16*slot) of dataMom_d (the full [locT*16*nLoop x Nmom] array) are written; the rows of the
 * other slots keep what they held.  The OPT plan uses it to leave reflected slots out of the projection (see
 * mugiq_hip_reflect_momentum_space). */
int mugiq_hip_convert_and_project_slots(void *dataMom_d, const void *dataPos_d, int nLoop, const int *slots_h, int nSlots,
                                        const int *momMatrix_h, int Nmom, int FTSign, const int localL[4], const int totalL[4],
                                        const int commCoord[4], int precision, void *workspace_d, size_t workspace_bytes, void *stream);

/* How the fused reorder + x step of the two calls above is dispatched for a shape (new; host only, no device work): the decisions
 * the launcher itself takes, through the same helper.  Same validation and the same environment switches (MUGIQ_HIP_EO_MFMA,
 * MUGIQ_HIP_EO_TILES_PER_WG) as the compute calls; nData = 16 * (number of slots projected). */
#define MUGIQ_HIP_PROJECT_FORM_GENERAL 0   /* eo_dft_x_kernel: any Lx, one tile per workgroup, tiles cut along t */
#define MUGIQ_HIP_PROJECT_FORM_PIPELINED 1 /* eo_dft_x_pipelined_kernel: a workgroup walks tilesPerWg tiles, prefetching the next */
#define MUGIQ_HIP_PROJECT_FORM_MFMA 2      /* eo_dft_x_mfma_kernel<nks, mb>: the same walk, sums on the fp64 matrix pipe */
typedef struct MugiqHipProjectPlan_s {
  int form;          /* MUGIQ_HIP_PROJECT_FORM_* */
  int nks, mb;       /* matrix pipe: k-steps per wave (Lx / 8) and 16-row blocks per tile; 0 otherwise */
  int nPx;           /* distinct p_x of the momentum list */
  int tChunk;        /* time slices per tile */
  int nChunks;       /* tiles per y pair: ceil(Lt / tChunk) */
  int lastChunk;     /* time slices of the last chunk (< tChunk: ragged, general form only) */
  int tiles;         /* (Ly / 2) * nChunks */
  int tilesPerWg;    /* consecutive tiles a workgroup walks (1 in the general form) */
  int workgroupsX;   /* ceil(tiles / tilesPerWg): grid.x (grid.y = Lz, grid.z = nData) */
  int rowPasses;     /* passes of 64 rows over a full tile (2 tChunk rows) */
  int pxPasses;      /* passes of 8 distinct p_x */
  int stagingPieces; /* 64-entry pieces of a run of Lx checkerboard entries (general form: > 1 for Lx > 64) */
  int redOffset;     /* complex elements from the tile to the partial-sum area (0: in the tile's place) */
  long long ldsBytes;/* dynamic LDS of the x-step kernel */
} MugiqHipProjectPlan;
int mugiq_hip_convert_and_project_plan(const int *momMatrix_h, int Nmom, const int localL[4], int nData, int precision,
                                       MugiqHipProjectPlan *out);

/* Reflected displacement entries in momentum space (new; host arrays only, no device work).  With L^-_k(x) = eta conj(L^+_k(x - k mu))
 * (mugiq_hip_reflect_displaced_loop), the Fourier transform of the derived slot follows from that of its source slot:
 *   dst(p, ig, t) = eta(15-ig) exp(-+ i FTSign 2 pi p_mu k / totalL[mu]) conj( src(-p, ig, t) )      mu = x, y, z
 *   dst(p, ig, t) = eta(15-ig) conj( src(-p, ig, t +- k) )   (t periodic over totT)                   mu = t
 * upper signs for dstDispSign = "+" (derived from a "-" entry).  dataMom_bcast_h: the gathered array of
 * performMomentumProjection (lib/loop_mugiq.cpp:415-424: per time-rank slabs of t + locT*ig + locT*16*iL + locT*16*nLoop*im);
 * slot srcSlot must be complete, slot dstSlot is overwritten.  MUGIQ_HIP_ERROR_UNSUPPORTED if some momentum of the list has no
 * partner -p in it. */
int mugiq_hip_reflect_momentum_space(void *dataMom_bcast_h, int precision, int Nmom, const int *momMatrix_h, int FTSign,
                                     const int totalL[4], int nLoop, int locT, int totT, int dstSlot, int srcSlot, int dispDir,
                                     int dstDispSign, int length);

/* ==== f2: MG coarse path -- Loop_Mugiq::prolongateEvec (lib/loop_mugiq.cpp:277-319) = QUDA Transfer::P ============== */

/* A coarse-grid colour-spinor in QUDA's FLOAT2 order (what Eigsolve_Mugiq hands over when computeCoarse is set,
 * lib/loop_mugiq.cpp:482): nSpin = 4/spin_block_size = 2 chiralities, nColor = n_vec; complex index of (s, c) at
 * (parity, x_cb): parity*parity_offset + (s*nColor + c)*stride + x_cb, even-odd on the coarse lattice X. */
typedef struct MugiqHipCoarseField_s {
  void *data;
  int precision; /* 4 | 8 */
  int nSpin;     /* 2 */
  int nColor;    /* n_vec */
  int volumeCB;
  int stride;
  int X[4];      /* coarse lattice dims = fine dims / geo_block_size, all even */
  int64_t parity_offset;
} MugiqHipCoarseField;

/* One level of QUDA's Transfer: the block-orthonormal null vectors V as a field of the FINER side with a packed vector
 * index.  Finest level: FieldOrderCB<Float,4,3,n_vec,FLOAT2>, complex index of V(parity, x_cb; s, c, j) =
 * parity*parity_offset + ((3*s + c)*nVec + j)*stride + x_cb, spinBlockSize 2.  Coarse -> coarse levels: see
 * mugiq_hip_prolongate_coarse_batched.  V comes from QUDA's MG setup or from the engine's own (mugiq_hip_mg_setup, below: null vectors
 * by an early-stopped CG, packed by mugiq_hip_transfer_set_vectors and made block-orthonormal by mugiq_hip_block_orthonormalize); the
 * two are interchangeable, and mugiq_hip_transfer_orthonormality checks either. */
typedef struct MugiqHipTransfer_s {
  const void *V;
  int precision;       /* 4 | 8 */
  int nVec;            /* mg_param.n_vec[0], default 24 (tests/loop.cpp:492) */
  int geoBlockSize[4]; /* mg_param.geo_block_size[0], default 4^4 (tests/loop.cpp:471) */
  int spinBlockSize;   /* 2 (tests/loop.cpp:569) */
  int X[4];            /* local dims of the finer side of this level */
  int stride;          /* volumeCB of the finer side + pad */
  int64_t parity_offset;
} MugiqHipTransfer;

/* fine_h[n](x; s, c) = sum_j V(x; s, c, j) * coarse_h[n](X(x); s/spinBlockSize, j) for all n < nVec in one launch
 * (the reference prolongs one eigenvector per call, and again for every displacement entry: lib/loop_mugiq.cpp:482). */
int mugiq_hip_prolongate_batched(const MugiqHipSpinorField *fine_h, const MugiqHipCoarseField *coarse_h, int nVec,
                                 const MugiqHipTransfer *transfer, void *stream);
/* One COARSE -> COARSE level of the hierarchy (mg_env.transfer[lev], lev >= 1; Loop_Mugiq::prolongateEvec walks them from
 * the coarsest level up before the finest transfer, lib/loop_mugiq.cpp:306-311).  Both sides are coarse fields with
 * nSpin = 2: out_h[n](x; s, c) = sum_j V(x; s, c, j) * in_h[n](X(x); s, j), with `transfer` describing this level:
 * X = dims of the FINER of the two lattices (= out_h[n].X), geoBlockSize, nVec = in_h[n].nColor, spinBlockSize = 1, and
 * V = FieldOrderCB<Float, 2, out_h[n].nColor, nVec, FLOAT2>: complex index parity*parity_offset +
 * ((out.nColor*s + c)*nVec + j)*stride + x_cb.  All nVec eigenvectors in one launch. */
int mugiq_hip_prolongate_coarse_batched(const MugiqHipCoarseField *out_h, const MugiqHipCoarseField *in_h, int nVec,
                                        const MugiqHipTransfer *transfer, void *stream);
/* Ultra-local loop of the MG path without materialising the fine vectors:
 * loopData += sum_n (1/sigma_n) (P c_n)^dag G (P c_n).  loopPrecision as in the *_mixed entry points. */
int mugiq_hip_prolongate_contract_batched(void *loopData_d, int loopPrecision, const MugiqHipCoarseField *coarse_h,
                                          const double *sigma_h, int nVec, const MugiqHipTransfer *transfer,
                                          void *stream);

/* ---- restriction R = P^dag (new): QUDA's Transfer::R, the adjoint of Transfer::P above.  The reference never calls it itself: its
 * computeCoarse mode (lib/eigsolve_mugiq.cpp:27-33) works on mg_env->diracCoarse, which QUDA builds from it (here:
 * mugiq_hip_compute_coarse_operator, below). ---------------------------------------------------------------------------------------- */
/* coarse_h[n](X; S, j) = sum_{x in aggregate X} sum_{s: s/spinBlockSize = S} sum_c conj(V(x; s, c, j)) g(s) fine_h[n](x; s, c) for all
 * n < nVec; g = 1, or for gamma5 != 0 the diagonal of g5 = Gamma_15 (mugiq_hip_get_gamma_tables).  Layouts, aggregate map and the
 * checks on `transfer` are those of mugiq_hip_prolongate_batched.  fine_h: one precision (4 | 8), FLOAT2 | FLOAT4, any stride; V and
 * the coarse fields share the transfer's precision, which may differ from the fine one.  Products and sums in fp64, one rounding on
 * the store, no atomics, a summation order fixed by the transfer alone: bitwise reproducible, and a vector restricted alone equals
 * the same vector restricted in any batch.  V is read once per block of 8 vectors. */
int mugiq_hip_restrict_batched(const MugiqHipCoarseField *coarse_h, const MugiqHipSpinorField *fine_h, int nVec,
                               const MugiqHipTransfer *transfer, int gamma5, void *stream);
/* The adjoint of mugiq_hip_prolongate_coarse_batched for one COARSE -> COARSE level (`transfer` as described there):
 * coarser_h[n](X; s, j) = sum_{x in X} sum_c conj(V(x; s, c, j)) finer_h[n](x; s, c).  Same numerics as above. */
int mugiq_hip_restrict_coarse_batched(const MugiqHipCoarseField *coarser_h, const MugiqHipCoarseField *finer_h, int nVec,
                                      const MugiqHipTransfer *transfer, void *stream);

/* The kernel forms of a finest-level transfer (new; host only, no device work): what mugiq_hip_prolongate_batched and
 * mugiq_hip_prolongate_contract_batched select for it (csrc/transfer_form.cpp, the one place that decides), under the same environment
 * switches, with their launch geometry, and the level geometry every MG kernel is handed.  transfer: checked as by the compute calls;
 * V is not read (any non-NULL value).  finePrecision / fineOrder: of the fine fields of the prolongation (0: the transfer's precision);
 * loopPrecision 0: the transfer's; nVec: the eigenvectors of the call. */
#define MUGIQ_HIP_PROLONG_FAMILY_MFMA 1            /* matrix pipe, one workgroup per aggregate (prolong_mfma_kernel) */
#define MUGIQ_HIP_PROLONG_FAMILY_VECTOR_STAGED 2   /* vector kernel, the V tile of 16 sites staged in LDS */
#define MUGIQ_HIP_PROLONG_FAMILY_VECTOR_GLOBAL 3   /* vector kernel, V read from global memory (fp64, n_vec > 53) */
#define MUGIQ_HIP_CONTRACT_FAMILY_COARSE_MFMA 1    /* coarse-grid plan V C V^dag, congruence on the matrix pipe */
#define MUGIQ_HIP_CONTRACT_FAMILY_COARSE_VECTOR 2  /* coarse-grid plan, congruence on the vector pipe */
#define MUGIQ_HIP_CONTRACT_FAMILY_DIRECT_STAGED 3  /* per-eigenvector kernel (prolong and contract on the spot), V tile in LDS */
#define MUGIQ_HIP_CONTRACT_FAMILY_DIRECT_GLOBAL 4  /* ... V read from global memory */
typedef struct MugiqHipTransferForm_s {
  int X[4], Xc[4], bs[4];           /* finer lattice, coarser lattice, aggregate */
  int aggVol, volumeCB, volumeCBc;
  int coarseNColor, coarseStride;   /* the coarser side's fields where the library lays them out itself (no pad) */
  long long coarseParityOffset;
  /* mugiq_hip_prolongate_batched */
  int prolongFamily, prolongThreads, prolongWorkgroups;
  int prolongPasses, prolongBlocksPerPass; /* matrix pipe: launches, blocks of eight eigenvectors per launch */
  long long prolongLdsBytes;
  long long prolongWorkspaceBytes;  /* the head of the per-stream workspace the call may take (whatever the family) */
  /* mugiq_hip_prolongate_contract_batched; 0 where the family does not use it */
  int contractFamily, contractThreads, contractWorkgroups; /* of the congruence (coarse plan) or the per-eigenvector kernel */
  int JC, SPR, NH;                  /* vector congruence: columns per lane chunk, sites per round, chunks per (site, chi, chi') */
  int outerB, glds;                 /* coarse plan: outer-product kernel instance; matrix-pipe congruence staged global -> LDS */
  long long contractLdsBytes, contractScratchBytes; /* scratch: pointer table, 1/sigma and C(X) of the coarse plan */
} MugiqHipTransferForm;
int mugiq_hip_transfer_form(const MugiqHipTransfer *transfer, int finePrecision, int fineOrder, int loopPrecision, int nVec,
                            MugiqHipTransferForm *out);

/* ==== host-side driver: the Loop_Mugiq / Displace classes of the reference ========================================= */

/* include/enum_mugiq.h:35-41.  calcType is parsed but never read by the reference's live code; here it selects
 * the execution plan: BASIC = the reference's own sequence (one displacement + one contraction launch per
 * eigenvector and step, lib/loop_mugiq.cpp:478-503); OPT and BLAS = eigenvector-batched contraction and the
 * fused displaced contraction (same results to rounding). */
#define MUGIQ_HIP_LOOP_CALC_TYPE_BLAS 0
#define MUGIQ_HIP_LOOP_CALC_TYPE_OPT_KERNEL 1
#define MUGIQ_HIP_LOOP_CALC_TYPE_BASIC_KERNEL 2

/* What Loop_Mugiq reads from QUDA's comm layer and MPI (lib/loop_mugiq.cpp:61-88,406-424) and what
 * exchangeGhostVec does (lib/contract_wrappers.cu:166-169), as callbacks so the host program owns the
 * transport (MPI in a MuGiq build; torch.distributed/RCCL in mugiq_amd; NULL comm = one process).
 * All callbacks return 0 on success. */
typedef struct MugiqHipComm_s {
  void *ctx;
  int rank, size;
  int grid[4];  /* comm_dim(d): ranks along x,y,z,t */
  int coord[4]; /* comm_coord(d) */
  /* Send `bytes` from send_d to the neighbour at coord[dim]+dir (dir = +1 | -1, periodic) and receive `bytes`
   * into recv_d from the neighbour at coord[dim]-dir.  Device pointers; ordered after prior work on `stream`
   * and complete (or stream-ordered) before later work on `stream`. */
  int (*sendrecv)(void *ctx, const void *send_d, void *recv_d, size_t bytes, int dim, int dir, void *stream);
  /* MPI_Reduce(SUM) over the ranks sharing coord[3] onto the one with coord[0..2] == 0 (COMM_SPACE,
   * lib/loop_mugiq.cpp:67,406).  Host buffers of n_real reals of `precision` bytes each. */
  int (*reduce_space)(void *ctx, const void *send_h, void *recv_h, size_t n_real, int precision);
  /* MPI_Gather over the ranks with coord[0..2] == 0, ordered by coord[3], root coord[3] == 0 (COMM_TIME,
   * lib/loop_mugiq.cpp:81,420-422).  recv_h is significant on the root only. */
  int (*gather_time)(void *ctx, const void *send_h, void *recv_h, size_t n_real_per_rank, int precision);
  /* MPI_Bcast from world rank 0 (lib/loop_mugiq.cpp:424) */
  int (*bcast)(void *ctx, void *buf_h, size_t n_real, int precision);
  /* Optional (both NULL or both set).  The OPT plan posts the eigenvector halos of ALL partitioned entries at the start
   * of a compute, in blocks of eigenvectors (about 2 GiB per message): for every block it issues, between group_begin and
   * group_end, one sendrecv per such entry -- all on the same stream, to different neighbours -- and the groups of
   * successive blocks follow each other on that stream.  A transport that can run the messages of a group concurrently
   * (different xGMI links: ncclGroupStart/End; MPI_Isend/Irecv + Waitall) may defer them until group_end(ctx, stream); one
   * without these members runs every sendrecv as it comes. */
  int (*group_begin)(void *ctx);
  int (*group_end)(void *ctx, void *stream);
  /* comm_dim_partitioned(d) beyond grid[d] > 1 (QUDA: comm_dim_partitioned_set(d), the `--partition` switch of its tests):
   * non-zero on an axis of extent 1 runs the PARTITIONED code path along it -- ghost zones, face packing, halo messages,
   * interior / boundary split, gauge borders from sendrecv -- with the rank as its own forward and backward neighbour, so
   * the halo machinery can be exercised (and timed) at full per-GPU size on one device.  The result equals the
   * unpartitioned one.  sendrecv must then be set even when size == 1.  Zero-initialise for the usual behaviour. */
  int partitioned[4];
} MugiqHipComm;

/* ---- a transport inside the library: the table above served by RCCL (csrc/comm_rccl.cpp) ---------------------------------
 * ncclSend / ncclRecv on the caller's stream inside ncclGroupStart / End for the halos (different neighbours = different xGMI
 * links at once), ncclReduce / ncclAllGather / ncclBroadcast over sub-communicators of the world one (ncclCommSplit) for the
 * COMM_SPACE / COMM_TIME steps of lib/loop_mugiq.cpp:61-88, 406-424 (host payloads staged through device buffers).  librccl is
 * loaded on first use.  Rank <-> coordinate map: QUDA's default (x slowest, t fastest).  One process per GPU; the device the
 * communicator lives on is the current device at creation.
 *   rank 0:        mugiq_hip_rccl_get_unique_id(id)           then hand the 128 bytes to every rank (MPI_Bcast, a file, a socket)
 *   every rank:    mugiq_hip_rccl_comm_create(&rc, id, rank, size, grid, partitioned)     (collective: ncclCommInitRank + 2 splits)
 *                  mugiq_hip_rccl_comm_fill(rc, &comm)        `comm` then goes wherever a MugiqHipComm goes
 *                  ...                                        mugiq_hip_rccl_comm_destroy(rc) once no loop object uses `comm` any more
 * A host that has an ncclComm_t already wraps it with mugiq_hip_rccl_comm_from_nccl (the communicator stays the host's).
 * `partitioned` as MugiqHipComm.partitioned (NULL = none).  Verified on hardware with one rank only (self-neighbour halos through
 * ncclSend / ncclRecv, tests/test_gpu_nccl.py): the pool this was built on has one GPU per box. */
typedef struct MugiqHipRcclComm_s MugiqHipRcclComm;
int mugiq_hip_rccl_get_unique_id(void *id128_out);
int mugiq_hip_rccl_comm_create(MugiqHipRcclComm **out, const void *id128, int rank, int size, const int grid[4], const int partitioned[4]);
int mugiq_hip_rccl_comm_from_nccl(MugiqHipRcclComm **out, void *ncclComm_world, const int grid[4], const int partitioned[4]);
int mugiq_hip_rccl_comm_fill(MugiqHipRcclComm *c, MugiqHipComm *out);
int mugiq_hip_rccl_comm_destroy(MugiqHipRcclComm *c);
/* Multi-path halos (off by default; needs more than two ranks).  A halo message goes to ONE neighbour, i.e. over one of a GPU's
 * seven xGMI links, while the links to the GPUs that are no neighbour on that axis idle: with this on, every sendrecv of a transfer
 * group is cut into 1 + R parts (R <= 6 ranks that are neither the origin nor the destination); part 0 travels directly, the others
 * through one relay each, first hops in one ncclGroup, second hops in the next, through a bounce buffer the communicator owns (about
 * the size of the group's messages).  Every rank must switch it the same way.  The schedule (a pure function of rank, grid, axis,
 * direction and size) is exposed for inspection: mugiq_hip_rccl_relay_plan lists what `rank` posts for one message -- phase 1 | 2,
 * kind 0 send from the send buffer, 1 receive into the receive buffer, 2 receive into the bounce area, 3 send from the bounce area,
 * peer, byte offset and length -- and returns the number of operations (tests/test_rccl_relay_plan_cpu.py delivers every byte with
 * it on a simulated network).  Never run on hardware (one-GPU boxes). */
int mugiq_hip_rccl_comm_set_multipath(MugiqHipRcclComm *c, int on);
int mugiq_hip_rccl_relay_plan(int rank, const int grid[4], int dim, int dir, size_t bytes, int max_ops, int *phase, int *kind, int *peer,
                              size_t *offset, size_t *len, size_t *bounce_bytes);

/* exchangeGhostVec(ColorSpinorField *x), lib/contract_wrappers.cu:166-169 (x->exchangeGhost(QUDA_INVALID_PARITY, nFace = 1, 0)):
 * fill the depth-1 ghost zones v->ghost[d][0 | 1] of every partitioned dimension (comm->grid[d] > 1 or comm->partitioned[d]), both directions,
 * through comm->sendrecv (one transfer group when the transport has group_begin / group_end).  The zones must be device
 * buffers of 2*12*faceCB complex each; comm == NULL (one process) is a no-op.  The faces are packed into the library's
 * per-stream workspace. */
int mugiq_hip_exchange_ghost_vec(const MugiqHipSpinorField *v, const MugiqHipComm *comm, void *stream);

/* ---- low-mode deflation of solutions (new; the step between the host's solver and a two-sided loop) ---------- */
/* dst_r <- dst_r - sum_n v_n sigma_n^-1 c_nr,  c_nr = sum_x v_n(x)^dag G src_r(x),  G = g5 (gamma5 != 0) or 1.
 * sigma_h NULL: sigma = 1 (with gamma5 = 0 and dst == src this is the orthogonal projector 1 - V V^dag).
 * overlaps_h (optional, [nEv][nVec] complex double): c_nr, global, identical on every rank.
 * comm NULL: one domain.  src may alias dst.
 * dst_h / src_h: nVec descriptors of one precision (4 | 8), which may differ from the eigenvectors'; order, geometry, stride and
 * parity offset as the eigenvectors'; nParity = 2.  The sums are taken in fp64 in a fixed order (bitwise reproducible); fp32 dst
 * are rounded once.  Cross-rank sum: comm->reduce_space, gather_time, a fixed-order sum on the root, bcast (every rank calls).
 * Blocking: with one domain (comm NULL or size 1) and overlaps_h NULL the call is stream-ordered and does not block the host;
 * otherwise it synchronises `stream` once, when the overlaps leave the device (and again after the global ones are back). */
int mugiq_hip_deflate_low_modes(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec,
                                const MugiqHipSpinorField *eVecs_h, const double *sigma_h, int nEv, int gamma5,
                                double *overlaps_h, const MugiqHipComm *comm, void *stream);
/* mugiq_hip_deflate_low_modes for an eigenvector set that lives on the coarsest level of the MG hierarchy (computeCoarse),
 * without ever storing v_n = P w_n:  dst_r <- dst_r - P [ sum_n w_n sigma_n^-1 c_nr ],  c_nr = <w_n, R(G src_r)>, which equals the
 * fine-level result for any V.  transfers_h[0 .. nCoarseLevels): as for mugiq_hip_loop_create_coarse_levels, finest first;
 * coarseEvecs_h: nEv fields on the coarsest level, of the transfers' precision.  sigma_h, overlaps_h ([nEv][nVec]), comm, aliasing
 * of src and dst, blocking and reproducibility: the contract of mugiq_hip_deflate_low_modes (aggregates never straddle ranks: R and
 * P need no communication).  One restriction, the overlaps and the combination on the coarsest level, the prolongation through the
 * coarse levels, and one last pass that reads V, reads and writes dst and subtracts (no fine intermediate).  Work memory (per-stream
 * workspace): nVec coarse vectors on every level, at least sum_l nVec * 4 * n_vec_l * volumeCB_l complex of the transfers' precision (each
 * rounded up to 256 bytes; on the coarsest level with the eigenvectors' own stride and parity offset, pads included), plus
 * 2 * nEv * nVec complex doubles. */
int mugiq_hip_deflate_low_modes_coarse(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec,
                                       const MugiqHipCoarseField *coarseEvecs_h, const double *sigma_h, int nEv,
                                       const MugiqHipTransfer *transfers_h, int nCoarseLevels, int gamma5, double *overlaps_h,
                                       const MugiqHipComm *comm, void *stream);

/* ==== the Wilson and Wilson-clover operators, the eigenpair check and a deflated CG (csrc/wilson.hip, csrc/clover.hip) ========= */
/* MuGiqEigOperator, include/enum_mugiq.h:22-25 (values identical), plus H = g5 M, which the reference does not have */
#define MUGIQ_HIP_EIG_OPERATOR_M 0
#define MUGIQ_HIP_EIG_OPERATOR_MDAG 1
#define MUGIQ_HIP_EIG_OPERATOR_MDAGM 2
#define MUGIQ_HIP_EIG_OPERATOR_MMDAG 3
#define MUGIQ_HIP_EIG_OPERATOR_H 4

/* Stands in for QUDA's DiracM / DiracMdag / DiracMdagM / DiracMMdag on a Wilson Dirac operator, as Eigsolve_Mugiq applies it
 * ((*mat)(w, v), lib/eigsolve_mugiq.cpp:301): dst_i = scale * A src_i, i < nVec, A one of the forms above of the UNIMPROVED Wilson
 * operator in kappa normalisation
 *   M psi(x) = psi(x) - kappa sum_mu [ (1 - g_mu) U_mu(x) psi(x+mu) + (1 + g_mu) U_mu^dag(x-mu) psi(x-mu) ],
 *   g_x, g_y, g_z, g_t = Gamma_1, Gamma_2, Gamma_4, Gamma_8 of mugiq_hip_get_gamma_tables ("g1" .. "g4"), g5 = Gamma_15.
 * The clover term is added by mugiq_hip_wilson_clover_apply below; no twisted mass, no even-odd preconditioning.
 * Links are applied as stored (boundary phases and anisotropy are
 * the host's business; they need not be unitary), the contract of mugiq_hip_perform_covariant_displacement_vector; the gauge
 * precision (4 | 8) is independent of the spinors'.  `scale`: e.g. the reference's 0.25 / kappa^2 for QUDA_MASS_NORMALIZATION (:302).
 * dst_h / src_h: nVec descriptors each, one precision, order, geometry, stride and parity offset; no dst may overlap any src.
 * Arithmetic in the fields' precision; pads are neither read into a result nor written.
 * comm NULL: one domain.  Otherwise commDim[d] = (comm->grid[d] > 1 || comm->partitioned[d]) as for the displacement: the off-face
 * neighbour comes from src->ghost[d][0 | 1] (required), which this call fills itself through comm->sendrecv (one transfer group per
 * block of 8 vectors), the link at x - mu from the border of the extended gauge field: R[d] >= 1 there, MUGIQ_HIP_ERROR_INVALID_ARGUMENT
 * otherwise.  MdagM / MMdag are two applications with a halo exchange of the intermediate, which lives in the per-stream workspace. */
int mugiq_hip_wilson_apply(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec, const MugiqHipGaugeField *gauge,
                           double kappa, int opType, double scale, const MugiqHipComm *comm, void *stream);

/* Eigsolve_Mugiq::computeEvals, lib/eigsolve_mugiq.cpp:289-315, restated literally for A = the form opType of the operator above:
 *   w = A v_n (times 0.25 / kappa^2 if massNormalization);  lambda_n = v_n^dag w / ||v_n||;  r_n = ||lambda_n v_n - w||
 * -- the division is by ||v||, not ||v||^2, as in the reference (:303; the two agree for normalised vectors only).
 * lambda_h[nEv] complex double (re, im), residual_h[nEv]; sigma_h[nEv] = sqrt(Re lambda) for MdagM / MMdag (:309-312), = Re lambda
 * WITH its sign for H (what a two-sided loop needs), untouched (may be NULL) for M and Mdag.
 * The eigenvectors (any storage) are only read, ghost zones included.  Inner products and norms in fp64, summed in a fixed order
 * and over the ranks as mugiq_hip_deflate_low_modes does: identical on every rank, bitwise reproducible.  Work memory: 24 vectors
 * of the eigenvectors' storage in the per-stream workspace, whatever nEv.  Blocks the host (two reads per block of 8 vectors). */
int mugiq_hip_compute_evals(const MugiqHipSpinorField *eVecs_h, int nEv, const MugiqHipGaugeField *gauge, double kappa, int opType,
                            int massNormalization, double *lambda_h, double *residual_h, double *sigma_h, const MugiqHipComm *comm,
                            void *stream);

/* Eigsolve_Mugiq::projectVector, lib/eigsolve_mugiq.cpp:340-348: out = sum_i v_i <v_i, in>, on the overlap and update kernels of
 * mugiq_hip_deflate_low_modes.  out, in: fp64, one layout (the eigenvectors' order, geometry, stride, parity offset), not aliased. */
int mugiq_hip_project_vector(const MugiqHipSpinorField *out, const MugiqHipSpinorField *in, const MugiqHipSpinorField *eVecs_h, int nEv,
                             const MugiqHipComm *comm, void *stream);

/* Stands in for the invertQuda call the deflated recipe needs ("Two-sided loops"): x_r = M^-1 b_r, r < nVec, by CG on
 * M^dag M x = M^dag b.  A correctness-first solver for that recipe and for tests -- plain CG in fp64, no preconditioner, two host
 * reads per iteration -- not a rival of a multigrid solve.
 * nEv > 0: the start vector is the low-mode part x0 = sum_n v_n sigma_n^-1 (v_n^dag g5 b) with (v_n, sigma_n) eigenpairs of
 * H = g5 M (eigenvectors of any storage, layout as x and b); nEv = 0: x0 = 0.  Right-hand sides advance in blocks of 8 through the
 * batched operator, each with its own scalars; a converged one is no longer touched.  Stops when ||M^dag b - M^dag M x|| <=
 * tol ||M^dag b|| (recursive residual); iters_out[r] = iterations taken, relres_out[r] = the TRUE ||b - M x|| / ||b||, recomputed
 * with one more application (0 for b = 0, which returns x = 0 in 0 iterations).  MUGIQ_HIP_ERROR_NOT_CONVERGED if a right-hand side
 * reaches maxIter first: x and both outputs are filled all the same.
 * x_h, b_h: fp64, one layout, no x overlapping any b; they need no ghost zones.  All scalars come from fixed-order fp64 sums
 * (and the cross-rank sum of the deflation): two runs give identical bits and iteration counts.  Work memory: 32 fp64 vectors. */
int mugiq_hip_wilson_solve(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                           double kappa, const MugiqHipSpinorField *eVecs_h, const double *sigma_h, int nEv, double tol, int maxIter,
                           int *iters_out, double *relres_out, const MugiqHipComm *comm, void *stream);

/* ---- the clover term (new; the reference's tests load one through loadCloverQuda before anything else) ------------------------------
 * With gamma matrices and g5 as above, sign and normalisation of Luescher-Sint-Sommer-Weisz:
 *   M_clov psi(x) = A(x) psi(x) - kappa sum_mu [ (1 - g_mu) U_mu(x) psi(x+mu) + (1 + g_mu) U_mu^dag(x-mu) psi(x-mu) ]
 *   A(x)       = 1 + i coeff sum_{mu<nu} sigma_{mu nu} (x) Fhat_{mu nu}(x),     coeff = kappa * c_sw  (QUDA's clover_coeff)
 *   sigma_mn   = (i/2) [g_m, g_n]
 *   Fhat_mn(x) = (1/8) (Q_mn(x) - Q_mn(x)^dag)                                   (no trace removed)
 *   Q_mn(x)    =   U_m(x)       U_n(x+m)       U_m^dag(x+n)  U_n^dag(x)
 *                + U_n(x)       U_m^dag(x-m+n) U_n^dag(x-m)  U_m(x-m)
 *                + U_m^dag(x-m) U_n^dag(x-m-n) U_m(x-m-n)    U_n(x-n)
 *                + U_n^dag(x-n) U_m(x-n)       U_n(x+m-n)    U_m^dag(x)
 * Links are used as stored: U^dag is the conjugate transpose, not the inverse, and links need not be unitary; boundary phases and
 * anisotropy stay the host's business, as for the hopping term.  g5 is diagonal, so A commutes with it and is block diagonal: two
 * Hermitian 6 x 6 blocks per site, block 0 on spins 0, 1 and block 1 on spins 2, 3, index inside a block i = spin_local*3 + colour.
 * Hence M_clov^dag = g5 M_clov g5, and every form of the operator below works as for the unimproved one.
 *
 * MugiqHipCloverField: local sites only (the term is site-local: no border, no halo).  Packed storage, 72 reals per site, as 36 PAIRS
 * of reals of `precision`; pair p of (parity, x_cb) is at pair index
 *   parity*parity_offset + p*stride + x_cb                    (a wavefront's loads of one pair coalesce)
 * with, for block b = 0 | 1:
 *   p = 18*b + q,     q = 0, 1, 2:    (A_{2q,2q}, A_{2q+1,2q+1})         the real diagonal, two entries to a pair
 *   p = 18*b + 3 + l, l = i*(i-1)/2 + j, 0 <= j < i < 6:  (Re A_ij, Im A_ij)   the strictly-lower triangle, row by row:
 *                     (1,0) (2,0) (2,1) (3,0) (3,1) (3,2) (4,0) .. (4,3) (5,0) .. (5,4);    A_ji = conj(A_ij).
 * A host that has its own clover term fills the buffer itself; the supported route is mugiq_hip_compute_clover. */
typedef struct MugiqHipCloverField_s {
  void *data;
  int precision;         /* 4 | 8; must equal the gauge precision of the operator call it is passed to */
  int X[4];              /* local dims, all even */
  int volumeCB;
  int stride;            /* volumeCB + pad */
  int64_t parity_offset; /* pairs between the two parities, >= 36*stride */
} MugiqHipCloverField;

/* bytes of a pad-0 field: volumeCB * 36 pairs * 2 parities * 2 reals */
size_t mugiq_hip_clover_bytes(const int X[4], int precision);
/* allocate (zeroed, pad 0) and describe; release with mugiq_hip_free_clover */
int mugiq_hip_alloc_clover(MugiqHipCloverField *clover, const int X[4], int precision);
int mugiq_hip_free_clover(MugiqHipCloverField *clover);
/* Fill `clover` with A(x) of the definition above from the border-extended gauge field (either precision; fp64 arithmetic whatever the
 * storages, rounded once on the store).  One lattice site per lane, one plane at a time.  Links are addressed as by the stencil, always
 * in the extended field: R[d] >= 1 supplies x +- m across a face and the edge and corner regions supply the diagonal neighbours
 * x-m+n, x+m-n, x-m-n (mugiq_hip_create_extended_gauge fills them); R[d] = 0 wraps.  A partitioned dimension (comm, as for
 * mugiq_hip_wilson_apply) with R[d] = 0 is MUGIQ_HIP_ERROR_INVALID_ARGUMENT.  No communication of its own.  Pads are not written. */
int mugiq_hip_compute_clover(const MugiqHipCloverField *clover, const MugiqHipGaugeField *gauge, double coeff, const MugiqHipComm *comm,
                             void *stream);

/* mugiq_hip_wilson_apply, mugiq_hip_compute_evals and mugiq_hip_wilson_solve for M_clov: each is its twin plus `clover`.  clover NULL:
 * the unimproved operator, through the same code as the twin (identical bits).  Otherwise its geometry must be the spinors', its
 * precision the gauge field's (the operator's precision), stride >= volumeCB, parity_offset >= 36*stride: MUGIQ_HIP_ERROR_INVALID_ARGUMENT
 * if not.  The term is applied inside the one stencil kernel (the accumulators start as A psi instead of psi), in the spinors' precision.
 * For the solver, (v_n, sigma_n) are eigenpairs of H = g5 M_clov. */
int mugiq_hip_wilson_clover_apply(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec, const MugiqHipGaugeField *gauge,
                                  const MugiqHipCloverField *clover, double kappa, int opType, double scale, const MugiqHipComm *comm,
                                  void *stream);
int mugiq_hip_compute_evals_clover(const MugiqHipSpinorField *eVecs_h, int nEv, const MugiqHipGaugeField *gauge,
                                   const MugiqHipCloverField *clover, double kappa, int opType, int massNormalization, double *lambda_h,
                                   double *residual_h, double *sigma_h, const MugiqHipComm *comm, void *stream);
/* Eigsolve_Mugiq::computeEvals (lib/eigsolve_mugiq.cpp:289-315) for the computeCoarse branch (:27-33), where the reference runs the same
 * check on mg_env->diracCoarse: the eigenvectors w_n live on the coarsest level (coarseEvecs_h, transfers_h[0 .. nCoarseLevels) as for
 * mugiq_hip_deflate_low_modes_coarse) and the coarse operator is the Galerkin operator M_c = R M P, M_c^dag = R M^dag P, with M the
 * Wilson (clover NULL) or Wilson-clover operator above.  Forms: M, Mdag, MdagM = M_c^dag M_c and MMdag = M_c M_c^dag (QUDA's DiracMdagM on
 * DiracCoarse, not R MdagM P), H = R g5 M P.  lambda_n = w_n^dag A_c w_n / ||w_n||, r_n = ||lambda_n w_n - A_c w_n||, sigma and
 * massNormalization as for mugiq_hip_compute_evals.  Blocks of 8: prolongation, one call of the batched stencil with its halo exchange,
 * restriction; scalars are fixed-order fp64 sums, summed over the ranks as mugiq_hip_deflate_low_modes does.  Work memory (per-stream
 * workspace): 16 fine vectors of the transfers' precision (FLOAT2, with ghost zones on partitioned axes), 16 coarse vectors on every
 * level, and room for 8 packed level-1 vectors in fp64.  Blocks the host (two reads per block). */
int mugiq_hip_compute_evals_coarse(const MugiqHipCoarseField *coarseEvecs_h, int nEv, const MugiqHipTransfer *transfers_h, int nCoarseLevels,
                                   const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover, double kappa, int opType,
                                   int massNormalization, double *lambda_h, double *residual_h, double *sigma_h, const MugiqHipComm *comm,
                                   void *stream);
int mugiq_hip_wilson_clover_solve(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                                  const MugiqHipCloverField *clover, double kappa, const MugiqHipSpinorField *eVecs_h, const double *sigma_h,
                                  int nEv, double tol, int maxIter, int *iters_out, double *relres_out, const MugiqHipComm *comm,
                                  void *stream);

/* ---- the explicit Galerkin coarse operator (new; csrc/coarse_op.hip): what QUDA's DiracCoarse is to the reference's computeCoarse branch
 * (lib/eigsolve_mugiq.cpp:27-33) -- nine dense N x N matrices per coarse site, N = 2 n_vec, built once per configuration, so that an
 * application of M_c = R M P reads those matrices and never walks the fine lattice.
 *
 * Definitions.  M is the fine operator of mugiq_hip_wilson_clover_apply,
 *   M = A(x) - kappa sum_mu [ (1 - g_mu) U_mu(x) delta_{x+mu} + (1 + g_mu) U_mu^dag(x-mu) delta_{x-mu} ],   A = 1 without a clover field,
 * links applied as stored (U^dag: the conjugate transpose), and V the null vectors of a FINEST-level MugiqHipTransfer (spinBlockSize 2).
 * Row index r = S*n_vec + j, the coarse field's (s*nColor + c).  With V^dag(x) = sum_{s: s/2 = S} sum_c conj V(x; s, c, j) ... and
 * V(x') = V(x'; s', c', j'), s'/2 = S', for the coarse site X (an aggregate):
 *   Xd(X)    = sum_{x in X} V^dag(x) A(x) V(x)
 *              - kappa sum_mu sum_{x in X, x+mu in X} V^dag(x) (1 - g_mu) U_mu(x) V(x+mu)
 *              - kappa sum_mu sum_{x in X, x-mu in X} V^dag(x) (1 + g_mu) U_mu^dag(x-mu) V(x-mu)
 *   Y+_mu(X) = - kappa sum_{x in X, x+mu not in X} V^dag(x) (1 - g_mu) U_mu(x) V(x+mu)
 *   Y-_mu(X) = - kappa sum_{x in X, x-mu not in X} V^dag(x) (1 + g_mu) U_mu^dag(x-mu) V(x-mu)
 *   (M_c in)(X) = Xd(X) in(X) + sum_mu [ Y+_mu(X) in(X+mu) + Y-_mu(X) in(X-mu) ]
 * Membership is by aggregate, after the periodic wrap; coarse extents are even (>= 2), so a hop that leaves the block lands in another
 * aggregate.  With coarse extent 2, X+mu = X-mu: Y+ and Y- stay separate matrices, defined by the direction of the hop.  kappa is
 * folded in: a new kappa means a new build.
 *   M_c^dag: the explicit adjoint of the stored matrices,
 *     (M_c^dag in)(X) = Xd(X)^dag in(X) + sum_mu [ Y-_mu(X+mu)^dag in(X+mu) + Y+_mu(X-mu)^dag in(X-mu) ]  = R M^dag P for ANY V (no
 *     block-orthonormality assumed);
 *   H_c = R g5 M P = G5 M_c, G5 = diag(g5(S)): +1 on chirality 0, -1 on chirality 1;
 *   MdagM = M_c^dag M_c and MMdag = M_c M_c^dag: products of the coarse operators, as in mugiq_hip_compute_evals_coarse.
 *
 * Storage: matrix-contiguous, no pad.  The complex element (m, r, c) of site (parity, x_cb) is at
 *   ((parity*volumeCB + x_cb)*9 + m)*N*N + r*N + c,       m = 0: Xd,  m = 1 + 2 mu: Y+_mu,  m = 2 + 2 mu: Y-_mu
 * (32^4 with 4^4 aggregates and n_vec 24 in fp64: 1.36 GB).
 *
 * Limits: a SINGLE DOMAIN (a comm with size > 1 or any partitioned axis: MUGIQ_HIP_ERROR_UNSUPPORTED, before any device work).  The
 * operator of a coarse -> coarse transfer is built from this one by mugiq_hip_compute_coarse_operator_coarse (below) and lives in the same
 * struct: application, eigenpair check and eigensolver do not know the level.  Process grids are served by the entry points of their own
 * further down -- mugiq_hip_compute_coarse_operator_grid, mugiq_hip_coarse_apply_grid and mugiq_hip_compute_evals_coarse_operator_grid,
 * with a MugiqHipCoarseHalo beside the operator -- and, through the fine lattice, by mugiq_hip_compute_evals_coarse. */
typedef struct MugiqHipCoarseOperator_s {
  void *data;
  int precision; /* 4 | 8: the transfer's (and the coarse fields') */
  int nVec;      /* n_vec of the transfer; N = 2*nVec */
  int X[4];      /* coarse lattice dims, all even */
  int volumeCB;
  double kappa;  /* of the last build (informational) */
  int hasClover; /* the last build had a clover field */
} MugiqHipCoarseOperator;

/* bytes of the nine matrices of every site: volume * 9 * N^2 complex of `precision` */
size_t mugiq_hip_coarse_operator_bytes(const int X[4], int nVec, int precision);
/* allocate (zeroed) and describe; release with mugiq_hip_free_coarse_operator */
int mugiq_hip_alloc_coarse_operator(MugiqHipCoarseOperator *op, const int X[4], int nVec, int precision);
int mugiq_hip_free_coarse_operator(MugiqHipCoarseOperator *op);
/* Fill `op` from the definitions above.  transfer: a finest-level one, whose precision and n_vec are the operator's and whose coarse
 * lattice is op->X; gauge (either precision; R[d] = 0 wraps, links addressed as by the stencil) and clover (NULL | the gauge field's
 * precision) as for mugiq_hip_wilson_clover_apply.  fp64 arithmetic whatever the storages, one rounding on the store, no atomics, a
 * summation order fixed by the transfer alone: two builds give identical bits.  One workgroup per aggregate and matrix, V(x) and
 * K(x) V(x') staged in LDS; a once-per-configuration cost.  Sets op->kappa and op->hasClover. */
int mugiq_hip_compute_coarse_operator(MugiqHipCoarseOperator *op, const MugiqHipTransfer *transfer, const MugiqHipGaugeField *gauge,
                                      const MugiqHipCloverField *clover, double kappa, const MugiqHipComm *comm, void *stream);
/* dst_i = scale * A_c src_i, i < nVec, A_c the form opType (MUGIQ_HIP_EIG_OPERATOR_*) of the coarse operator.  Coarse fields of the
 * operator's precision and lattice, any stride (one for all src, one for all dst); pads are neither read nor written; no dst may overlap
 * any src.  Blocks of 8 vectors: the matrices are read once per block.  Sums in fp64, one rounding on the store; a vector applied alone
 * equals the same vector applied in any batch, bit for bit.  The intermediate of MdagM / MMdag (8 vectors) lives in the per-stream
 * workspace. */
int mugiq_hip_coarse_apply(const MugiqHipCoarseField *dst_h, const MugiqHipCoarseField *src_h, int nVec, const MugiqHipCoarseOperator *op,
                           int opType, double scale, const MugiqHipComm *comm, void *stream);
/* The output components per workgroup -- 16, 32 or 64 -- one launch of the application's kernel takes for nVec vectors on this operator: the
 * answer of the one rule every launch asks (32 where the 64-output grid, 2 volumeCB x ceil(nVec / 8) x ceil(2 n_vec / 64) workgroups, would
 * have fewer than 512, else 64), under MUGIQ_HIP_COARSE_APPLY_OUT as the launches read it.  Host only: no device work, no launch; op->data
 * is not read, so a described geometry will do.  The results do not depend on the form, bit for bit.  0 with the last error set for an
 * operator mugiq_hip_coarse_apply would refuse or nVec < 1.  (A normal form applies in blocks of 8; the MG solvers pass at most 8.) */
int mugiq_hip_coarse_apply_outputs(const MugiqHipCoarseOperator *op, int nVec);
/* lambda, r and sigma of mugiq_hip_compute_evals_coarse (lib/eigsolve_mugiq.cpp:289-315) with A_c applied by mugiq_hip_coarse_apply:
 * massNormalization scales by 0.25 / op->kappa^2.  The same fixed-order fp64 scalar kernels; work memory: 8 coarse vectors and the
 * scalars in the operator workspace of the stream.  Blocks the host (two reads per block of 8). */
int mugiq_hip_compute_evals_coarse_operator(const MugiqHipCoarseField *coarseEvecs_h, int nEv, const MugiqHipCoarseOperator *op, int opType,
                                            int massNormalization, double *lambda_h, double *residual_h, double *sigma_h,
                                            const MugiqHipComm *comm, void *stream);

/* ---- the explicit coarse operator on a process grid (new; csrc/coarse_op.hip).  Xd, Y+-_mu, M_c and M_c^dag are the definitions above on
 * the GLOBAL lattice.  A rank owns the aggregates of its local fine lattice: local fine extents are multiples of the block size and local
 * coarse extents are even, so rank offsets are even and local parity is global parity.  MugiqHipCoarseOperator holds the matrices of the
 * local coarse sites, unchanged.  M_c of a site on a face reads the neighbour rank's coarse vector; M_c^dag reads the neighbour rank's
 * MATRIX as well, Y+_mu(X-mu)^dag for X on the local low face and Y-_mu(X+mu)^dag for X on the high face.  Those matrices are kept in a
 * MugiqHipCoarseHalo, filled once by the build.
 *
 * Face-site ordering (every face buffer of these calls, fine or coarse): a site with coordinates c on a face of axis mu (c[mu] = 0 or
 * X[mu] - 1) and parity p = (c0 + c1 + c2 + c3) & 1 has the face index p*faceCB + (l >> 1), faceCB = volumeCB / X[mu], l the
 * lexicographic index of the three other coordinates with the lowest axis fastest (QUDA's ghostFaceIndex at depth 1).  A site and the
 * neighbour-rank site it hops to share their three other coordinates, hence (l >> 1); their parities differ.
 *   Yback[mu]: Y+_mu of the BACKWARD neighbour's high-face sites, Yfwd[mu]: Y-_mu of the FORWARD neighbour's low-face sites; each
 *   2*faceCB matrices of N*N complex in the operator's precision, matrix-contiguous: element (r, c) of face site f at (f*N + r)*N + c.
 * Both NULL on an axis the halo was not built for (dims[mu] == 0).  With a rank as its own neighbour (MugiqHipComm.partitioned) the
 * halo holds copies of the rank's own matrices.
 *
 * These three calls serve a grid, and on top of them mugiq_hip_coarse_gram_grid, mugiq_hip_coarse_eigensolve_grid and the two-grid fp64
 * mugiq_hip_mg_precondition_grid / mugiq_hip_mg_solve_grid (further down).  Every other MG solve entry point (three levels, mixed,
 * deflated), mugiq_hip_mg_setup, the coarse deflation and mugiq_hip_compute_coarse_operator_coarse stay single-domain and refuse a
 * partitioned comm, as do the three single-domain calls above and mugiq_hip_coarse_eigensolve, mugiq_hip_coarse_gram and
 * mugiq_hip_coarse_rotate.  The exchange is not overlapped with interior work. */
typedef struct MugiqHipCoarseHalo_s {
  void *Yback[4], *Yfwd[4];
  int precision; /* of the operator it belongs to */
  int nVec;
  int X[4];      /* local coarse lattice of that operator */
  int volumeCB;
  int dims[4];   /* != 0: built for a partitioned axis mu */
} MugiqHipCoarseHalo;
/* bytes of all face matrices: sum over dims[mu] != 0 of 2 * (volume / X[mu]) * N^2 complex of `precision`; 0 for arguments the
 * allocation would refuse */
size_t mugiq_hip_coarse_halo_bytes(const int X[4], int nVec, int precision, const int dims[4]);
/* allocate (zeroed) for the geometry, n_vec and precision of `op` on the axes dims[mu] != 0; release with mugiq_hip_free_coarse_halo */
int mugiq_hip_alloc_coarse_halo(MugiqHipCoarseHalo *halo, const MugiqHipCoarseOperator *op, const int dims[4]);
int mugiq_hip_free_coarse_halo(MugiqHipCoarseHalo *halo);
/* mugiq_hip_compute_coarse_operator on a process grid; collective.  gauge: border-extended with R >= 1 on every partitioned axis, as for
 * mugiq_hip_wilson_clover_apply; clover: the local field.  On every partitioned axis the two faces of V (12 n_vec complex per face site)
 * go to the neighbours in one transfer group, into the per-stream workspace; a hop that leaves the local lattice reads V(x +- mu) from
 * there and its link from the border, every sum in the order of the single-domain build, so a rank's matrices are the bits of its slice
 * of the single-domain operator.  Then Y+_mu of the high face and Y-_mu of the low face are packed and exchanged into `halo` (a second
 * group).  Checks, before any device work: NULL op / transfer; comm->sendrecv NULL on a partitioned comm; an operator with an odd extent;
 * halo NULL on a partitioned comm, or of another geometry, n_vec or precision than op, or not built for a partitioned axis; a gauge
 * border of 0 on a partitioned axis; everything mugiq_hip_compute_coarse_operator checks.  With nothing partitioned (comm NULL, or one
 * rank without a forced axis) halo may be NULL and the call is mugiq_hip_compute_coarse_operator: the same launch, the same bits. */
int mugiq_hip_compute_coarse_operator_grid(MugiqHipCoarseOperator *op, const MugiqHipCoarseHalo *halo, const MugiqHipTransfer *transfer,
                                           const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover, double kappa,
                                           const MugiqHipComm *comm, void *stream);
/* mugiq_hip_coarse_apply on a process grid; collective, all five forms.  Per kernel launch (one for M, M^dag and H on all nVec vectors;
 * two per block of 8 for MdagM and MMdag, whose intermediate is exchanged as well) the faces of the input vectors are packed -- N complex
 * per face site and vector, the face index fastest, then the component, the parity and the vector -- and sent in ONE message per
 * partitioned axis and direction, inside group_begin / group_end where the comm has them; then the one launch of the application follows,
 * whose hops off the rank read the received faces and, for M^dag, the halo's matrices.  Nothing overlaps the exchange.  The sums and
 * their order are those of mugiq_hip_coarse_apply: the result is the bits of the rank's slice of the single-domain result.  Work memory
 * (send and receive faces, the intermediate): the per-stream workspace; pads are neither read nor written.  Checks as above (no gauge)
 * plus those of mugiq_hip_coarse_apply; nothing partitioned: halo may be NULL, the call is mugiq_hip_coarse_apply. */
int mugiq_hip_coarse_apply_grid(const MugiqHipCoarseField *dst_h, const MugiqHipCoarseField *src_h, int nVec, const MugiqHipCoarseOperator *op,
                                const MugiqHipCoarseHalo *halo, int opType, double scale, const MugiqHipComm *comm, void *stream);
/* mugiq_hip_compute_evals_coarse_operator on a process grid: A_c by mugiq_hip_coarse_apply_grid, the fixed-order fp64 sums of every rank
 * added over the ranks in a fixed order (reduce_space, gather_time and bcast, required with size > 1): identical values on every rank. */
int mugiq_hip_compute_evals_coarse_operator_grid(const MugiqHipCoarseField *coarseEvecs_h, int nEv, const MugiqHipCoarseOperator *op,
                                                 const MugiqHipCoarseHalo *halo, int opType, int massNormalization, double *lambda_h,
                                                 double *residual_h, double *sigma_h, const MugiqHipComm *comm, void *stream);

/* ---- the operator of a coarse -> coarse transfer (new; csrc/coarse_op2.hip): the coarsest level of a three-level hierarchy, where the
 * reference's Eigsolve_Mugiq computes its eigenvectors (MG_Mugiq takes n_level 2, 3 or 4: include/mg_mugiq.h:40-53;
 * lib/eigsolve_mugiq.cpp:135-152).
 *
 * Definition.  Let K_m(x), m = 0 .. 8, be the matrices of a coarse operator on the lattice X1 (m = 0: Xd, 1 + 2 mu: Y+_mu, 2 + 2 mu: Y-_mu),
 * of size N0 x N0, N0 = 2 nc, and V the null vectors of a coarse -> coarse MugiqHipTransfer on X1 (spinBlockSize 1, nc colours on its finer
 * side, nVec = nv, complex index ((nc*s + c)*nv + j)*stride + x_cb).  N1 = 2 nv, row index S*nv + j; E(x) is the N0 x N1 embedding
 * E[(s, c), (S', j')] = delta_{s S'} V(x; s, c, j'): the chirality is kept.  For the coarsest site X (an aggregate of geoBlockSize):
 *   Xd'(X)   = sum_{x in X} E(x)^dag K_0(x) E(x)
 *              + sum_mu sum_{x in X, x+mu in X} E(x)^dag K_{1+2mu}(x) E(x+mu)
 *              + sum_mu sum_{x in X, x-mu in X} E(x)^dag K_{2+2mu}(x) E(x-mu)
 *   Y'+_mu(X) = sum_{x in X, x+mu not in X} E(x)^dag K_{1+2mu}(x) E(x+mu)
 *   Y'-_mu(X) = sum_{x in X, x-mu not in X} E(x)^dag K_{2+2mu}(x) E(x-mu)
 * Membership is by aggregate, after the periodic wrap.  The forward and the backward term stay separate even where x+mu = x-mu (extent 2
 * on X1, or on the coarsest lattice).  Storage and application of the result are those of MugiqHipCoarseOperator; kappa and hasClover
 * are inherited from the input operator.  Nothing assumes that V is block-orthonormal.  By construction the result is R_1 M_c P_1
 * (= R_1 R_0 M P_0 P_1), its explicit adjoint R_1 M_c^dag P_1, and G5 M' = R_1 R_0 g5 M P_0 P_1.
 *
 * Checks, all before any device work: NULL arguments; a single domain (MUGIQ_HIP_ERROR_UNSUPPORTED); transfer->spinBlockSize == 1;
 * transfer->X == finerOp->X; stride >= volumeCB; parity_offset == 2 finerOp->nVec nVec stride exactly (the rule of
 * mugiq_hip_block_orthonormalize for the colours of a coarse V); the block sizes divide the extents and the coarsest extents are even;
 * op->X, op->nVec and op->precision are the transfer's; the three precisions are equal; op->data does not overlap finerOp->data.
 * Every nc <= 64 and nv <= 64 (the limits of the struct) is served.
 * Numerics: fp64 products and sums for either storage, one rounding on the store, no atomics, and a summation order fixed by the
 * transfer geometry alone (sites of the aggregate in lexicographic order; per site K_0, then +x, -x, ... -t): two builds give the same
 * bits on any stream.  Every K_m(x) is read from memory once per build: the four workgroups of a matrix own its chirality quadrants,
 * and a quadrant of the result needs that quadrant of K alone.  The input can itself be a result of this call (a fourth level); nothing
 * tests that. */
int mugiq_hip_compute_coarse_operator_coarse(MugiqHipCoarseOperator *op, const MugiqHipTransfer *transfer, const MugiqHipCoarseOperator *finerOp,
                                             const MugiqHipComm *comm, void *stream);

/* ---- a two-grid preconditioned flexible GCR on the fine operator (new; csrc/mg_solve.hip): the solve of the deflated recipe for every
 * stochastic source, for hosts that hold an MG hierarchy (V of a finest-level transfer and its explicit coarse operator).
 *
 * Definitions.  M is the operator of mugiq_hip_wilson_clover_apply (clover NULL: unimproved); M_c, P = mugiq_hip_prolongate_batched and
 * R = P^dag = mugiq_hip_restrict_batched those of the coarse-operator section above.  All inner products <a, b> = sum conj(a) b are fp64
 * fixed-order sums.
 *   MR step on (z, s):  t = M s,  d = <t, t>,  alpha = omega <t, s> / d if d > 0, else 0;  z += alpha s,  s -= alpha t.
 *   GCRfix(A, b, n):  x = 0, r = b; for k = 0 .. n-1:  p = r, q = A p;  c_j = <q_j, q> for all j < k, taken from the un-updated q
 *     (classical Gram-Schmidt, one pass);  p -= sum c_j p_j,  q -= sum c_j q_j;  nu = ||q||: if nu = 0 the step contributes nothing and
 *     stores a zero direction, otherwise p /= nu, q /= nu;  alpha = <q, r>,  x += alpha p,  r -= alpha q.  Returns x.
 *   K(r), the preconditioner:  z = 0, s = r;  nuPre MR steps;  if coarseIters > 0: e = GCRfix(M_c, R s, coarseIters), z += P e,
 *     s = r - M z (one application);  nuPost MR steps;  returns z.  K is homogeneous: K(c r) = c K(r) for real c > 0.
 *   Outer solve of M x = b:  x = 0, r = b; the recurrence of GCRfix with p = K(r), q = M p, the directions cleared after every nKrylov
 *     steps; stops at the first iteration with recursive ||r|| <= tol ||b||.  relres is the TRUE ||b - M x|| / ||b|| from one more
 *     application, history[i] the recursive relative residual after iteration i + 1;  b = 0 gives x = 0 in 0 iterations.
 * (alpha = <q, r> is formed as <q, r> / nu from the orthogonalised q before its normalisation, in the pass that orthogonalises it.)
 * Right-hand sides advance in blocks of at most 8 through the batched operators, each with its own scalars; a converged one is no longer
 * touched, and one solved alone equals the same one in any batch, bit for bit.
 *
 * Inside K nothing is read back: K is a fixed sequence of launches whose scalars (Gram-Schmidt coefficients, nu, alpha) stay in device
 * memory.  The outer loop blocks the host once per iteration (the residual norms of the block) and twice more per block (||b|| and the
 * true residual); *hostReads_out counts these reads.  No atomics: two runs give identical bits, iteration counts and histories.
 *
 * The defaults are first guesses that converge on the test fields; they are NOT tuned. */
typedef struct MugiqHipMgSolveParam_s {
  double tol;      /* > 0: recursive ||r|| <= tol ||b|| */
  int maxIter;     /* >= 0 outer iterations per right-hand side */
  int nKrylov;     /* 1 .. 16 stored directions of the outer GCR before a restart */
  int nuPre;       /* 0 .. 16 MR steps before the coarse-grid correction */
  int nuPost;      /* 0 .. 16 MR steps after it */
  double omega;    /* MR relaxation */
  int coarseIters; /* 0 .. 16 GCR steps on M_c; 0: no coarse-grid correction */
} MugiqHipMgSolveParam;
/* tol 1e-10, maxIter 1000, nKrylov 16, nuPre 0, nuPost 4, omega 1.0, coarseIters 8 */
int mugiq_hip_mg_solve_param_default(MugiqHipMgSolveParam *param);
/* z_i = K(r_i), i < nVec.  z_h, r_h: fp64 fields of one layout (FLOAT2 | FLOAT4, any stride; pads are neither read nor written), no z
 * overlapping any r; they need no ghost zones.  transfer: a finest-level one of precision 8 on the fields' lattice; coarseOp: the operator
 * built from it for this gauge field, clover field and kappa (precision 8).  tol and maxIter of `param` are checked but not used.
 * Limits, each refused before any device work: a single domain (MUGIQ_HIP_ERROR_UNSUPPORTED, as for the coarse operator) and a two-grid cycle
 * (three levels: mugiq_hip_mg_precondition_levels, below);
 * precision 4 anywhere in transfer, coarse operator or fields (MUGIQ_HIP_ERROR_UNSUPPORTED); parameters out of range, geometry mismatches
 * between fields, transfer and operator, a coarse operator built for another kappa or without / with the clover term of the call
 * (op->kappa, op->hasClover), a z overlapping an r or another z (MUGIQ_HIP_ERROR_INVALID_ARGUMENT).
 * Work memory, all from the per-stream operator workspace: 3 min(nVec, 8) fine vectors, (2 coarseIters + 2) min(nVec, 8) coarse vectors
 * and 0.6 MB of scalars; an allocation that fails is MUGIQ_HIP_ERROR_HIP, not an abort.  The workspace grows to 1.5 x a request that
 * does not fit and is kept for the stream (mugiq_hip_release_stream frees it). */
int mugiq_hip_mg_precondition(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                              const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfer,
                              const MugiqHipCoarseOperator *coarseOp, const MugiqHipMgSolveParam *param, const MugiqHipComm *comm, void *stream);
/* x_i = M^-1 b_i, i < nVec, by the outer solve above.  Fields and limits as for mugiq_hip_mg_precondition (x for z, b for r).
 * iters_out[nVec], relres_out[nVec]; history_out (may be NULL): history_out[i*historyStride + k] for k < iters_out[i], entries behind
 * that are not written, historyStride >= maxIter; hostReads_out (may be NULL): the blocking reads of this call, max(iters of the block)
 * + 2 per block of 8.  MUGIQ_HIP_ERROR_NOT_CONVERGED if a right-hand side reaches maxIter first: x and all outputs are filled all the same.
 * Work memory (per-stream operator workspace): (2 nKrylov + 4) min(nVec, 8) fine vectors -- the directions p_j and q_j, r, s, t and one
 * for P e -- (2 coarseIters + 2) min(nVec, 8) coarse vectors and 0.6 MB of scalars.  32^4, nKrylov 16, 8 right-hand sides: 58 GB are
 * used, and because the workspace grows to 1.5 x a request that does not fit, a first call on a stream allocates 87 GB (nKrylov 8: 32 GB
 * used, 48 GB allocated).  Size nKrylov from the allocation. */
int mugiq_hip_mg_solve(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                       const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfer, const MugiqHipCoarseOperator *coarseOp,
                       const MugiqHipMgSolveParam *param, int *iters_out, double *relres_out, double *history_out, int historyStride,
                       int *hostReads_out, const MugiqHipComm *comm, void *stream);

/* ---- the two-grid cycle and solve on a process grid (new; csrc/mg_solve.hip; tests/mg_solve_grid_ref.py restates the
 * recurrence rank by rank).  fp64, one coarse level, no deflation space.  Collective: every rank calls with its local fields.
 *
 * M is applied with its halo exchange (ghost zones as for mugiq_hip_wilson_clover_apply, gauge border R >= 1 on every partitioned axis),
 * M_c by the internals of mugiq_hip_coarse_apply_grid (coarseOp and halo from mugiq_hip_compute_coarse_operator_grid); R and P are local
 * to a rank, which owns whole aggregates.  Every inner product is the fixed-order sum of the rank, written into the rank's entry of a table
 * [rank][8][32] doubles on the device (rank order: x slowest, t fastest); a ring gather over every axis of extent > 1, t first, completes
 * the table on every rank -- sum_d (grid[d] - 1) calls of comm->sendrecv(.., d, +1, stream) on device buffers, straight from and into the
 * table, no host read and no pack kernel -- and one workgroup (mg_rank_sum_kernel) adds the entries in ascending rank order and forms what
 * the next kernel reads: the Gram-Schmidt coefficients, (nu, <q, r> / nu), the MR alpha, or the raw norms the host fetches.  The guards
 * nu > 0 and <t, t> > 0 act on the global sums.  Every rank adds the same numbers in the same order, so all ranks hold the same bits and
 * iteration counts, restarts, histories and statuses agree without a broadcast; the one read per outer iteration is the global value and
 * hostReads keeps its formula.  comm->reduce_space, gather_time and bcast are not used.  The sums are added per rank first, so on more than one
 * rank results agree with the single-domain solve to rounding, not bit for bit.  With one rank (forced axes only) no table exists,
 * nothing is gathered, and the results are the bits of mugiq_hip_mg_precondition / mugiq_hip_mg_solve; with nothing partitioned the calls
 * ARE those calls, launch for launch (halo may then be NULL).
 *
 * r_h of the cycle is read by the stencil in place: it needs ghost zones on every partitioned axis (refused otherwise, like src of
 * mugiq_hip_wilson_apply).  z_h, x_h and b_h need none.  Checks, each before any device work: comm NULL; those of
 * mugiq_hip_coarse_apply_grid (sendrecv NULL on a partitioned comm; halo NULL on a partitioned comm, of another operator, or not built for
 * a partitioned axis); comm->grid, coord, rank and size that do not describe one grid; a gauge border of 0 on a partitioned axis;
 * everything mugiq_hip_mg_precondition / mugiq_hip_mg_solve check (precision 4: MUGIQ_HIP_ERROR_UNSUPPORTED); gridInfo_out NULL.
 * Work memory: that of the single-domain calls, every fine vector followed by its ghost zones, plus the stencil's send buffers, one more
 * set of ghost zones per right-hand side of a block and the rank table (operator workspace), and the faces of the coarse application (the
 * per-stream workspace, reserved once per call).  The exchanges are not overlapped with interior work. */
typedef struct MugiqHipMgSolveGridInfo_s {
  int fineExchanges;   /* applications of M that exchanged ghost zones (0 with nothing partitioned) */
  int coarseExchanges; /* applications of M_c that exchanged faces */
  int rankSums;        /* sums that went through the rank table (0 on one rank: there is nothing to add) */
  int rankSumMessages; /* sendrecv calls made for them: rankSums * sum_d (grid[d] - 1) */
} MugiqHipMgSolveGridInfo;
int mugiq_hip_mg_precondition_grid(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                                   const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfer, const MugiqHipCoarseOperator *coarseOp,
                                   const MugiqHipCoarseHalo *halo, const MugiqHipMgSolveParam *param, const MugiqHipComm *comm, void *stream);
int mugiq_hip_mg_solve_grid(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                            const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfer, const MugiqHipCoarseOperator *coarseOp,
                            const MugiqHipCoarseHalo *halo, const MugiqHipMgSolveParam *param, int *iters_out, double *relres_out, double *history_out,
                            int historyStride, int *hostReads_out, MugiqHipMgSolveGridInfo *gridInfo_out, const MugiqHipComm *comm, void *stream);
/* The messages of the ring gather, for inspection (host only, no device): what the rank at `coord` of `grid` posts, in order.  Message m
 * is sendrecv(table + sendEntry[m], table + recvEntry[m], entries[m] entries, dim[m], +1): it sends the run that starts at entry
 * sendEntry[m] to the neighbour at coord[dim[m]] + 1 and receives the run at recvEntry[m] from the neighbour at coord[dim[m]] - 1 (an
 * entry: the 8 x 32 doubles of one rank).  Returns the number of messages, sum_d (grid[d] - 1), and fills the first maxOps of each
 * array that is not NULL; -1 for a NULL grid or coord, an extent < 1 or a coordinate outside its extent. */
int mugiq_hip_mg_rank_sum_plan(const int grid[4], const int coord[4], int maxOps, int *dim_out, int *sendEntry_out, int *recvEntry_out,
                               int *entries_out);

/* ---- the mixed-precision solve (new; csrc/mg_solve.hip): the cycle K in fp32 storage under the fp64 outer GCR, what QUDA's
 * --prec-sloppy / --prec-precondition give the reference's MG solve.  mugiq_hip_mg_precondition and mugiq_hip_mg_solve above do not
 * change: they keep refusing precision 4.
 *
 * Definitions.  K32 is K of the section above with every vector it stores -- s, t, w, the coarse directions, xc, rc, its input and its
 * result -- in fp32 storage, on a transfer and a coarse operator of precision 4, in the same sequence of launches.  The Krylov kernels
 * widen every load to fp64, form all products and sums in fp64 and round once on the store; the scalars (Gram-Schmidt coefficients, nu,
 * alpha, the partial sums) stay fp64 in device memory.  The stencil computes in the fields' precision (fp32), R, P and M_c sum in fp64.
 * Every promise of the fp64 path holds: a fixed summation order, no atomics, identical bits from two runs, a right-hand side alone equal
 * to the same one in any batch, pads neither read nor written; and K32(2^k r) = 2^k K32(r) bit for bit while nothing under- or overflows.
 *   Mixed solve of M x = b:  the outer solve above, unchanged and in fp64 -- operator applications, directions, residual, tol, history and
 *   the true residual -- with  p = widen(K32(round(r)))  in place of  p = K(r):  r is rounded to nearest into fp32, and the fp32 result is
 *   widened (exactly) straight into the direction slot.  r is not scaled: K is homogeneous, and a residual of 1e-10 ||b|| is far inside
 *   fp32's exponent range.  The outer GCR is flexible, so the rounding costs iterations at most, never accuracy: relres and x meet the
 *   bounds of mugiq_hip_mg_solve.
 * Nothing assumes that a V rounded to fp32 is block-orthonormal to better than fp32: the sloppy coarse operator is built from the rounded
 * V (mugiq_hip_transfer_convert, then mugiq_hip_compute_coarse_operator), so it is the Galerkin operator of that V. */

/* z_i = K32(r_i), i < nVec.  Arguments as for mugiq_hip_mg_precondition with z_h, r_h, transfer and coarseOp ALL of precision 4; gauge of
 * either precision, clover (NULL | of the gauge field's precision) as the stencil requires.  Refused before any device work: a process
 * grid or a partitioned axis (MUGIQ_HIP_ERROR_UNSUPPORTED); precision 8 in any of the four objects (MUGIQ_HIP_ERROR_INVALID_ARGUMENT: that is
 * mugiq_hip_mg_precondition); and everything else mugiq_hip_mg_precondition refuses (parameters, geometry, kappa, hasClover, overlaps).
 * Work memory (per-stream operator workspace): 3 min(nVec, 8) fine vectors and (2 coarseIters + 2) min(nVec, 8) coarse vectors, all fp32
 * -- half the bytes of mugiq_hip_mg_precondition per vector -- and the same 0.6 MB of fp64 scalars; an allocation that fails is
 * MUGIQ_HIP_ERROR_HIP, not an abort. */
int mugiq_hip_mg_precondition_sloppy(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                                     const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfer,
                                     const MugiqHipCoarseOperator *coarseOp, const MugiqHipMgSolveParam *param, const MugiqHipComm *comm,
                                     void *stream);
/* x_i = M^-1 b_i, i < nVec, by the mixed solve above.  x_h, b_h, gauge, clover, kappa, param and every output as for mugiq_hip_mg_solve
 * (fp64 fields; hostReads: max(iters of the block) + 2 per block of 8, nothing is read back inside K32; MUGIQ_HIP_ERROR_NOT_CONVERGED with
 * all outputs filled).  transferSloppy and coarseOpSloppy: the hierarchy in precision 4 (anything else: MUGIQ_HIP_ERROR_INVALID_ARGUMENT),
 * coarseOpSloppy built from transferSloppy for this kappa and clover term.  gaugeSloppy, cloverSloppy: the fields the cycle's stencil
 * reads, e.g. fp32 copies; both NULL: the cycle reads gauge and clover (the stencil takes fp32 spinors on fp64 links).  With a clover
 * field in the call they are given both or neither; without one cloverSloppy is NULL and gaugeSloppy optional; anything else is
 * MUGIQ_HIP_ERROR_INVALID_ARGUMENT.  The other limits are those of mugiq_hip_mg_solve.
 * Work memory (per-stream operator workspace): (2 nKrylov + 2) min(nVec, 8) fine vectors in fp64 -- the directions p_j and q_j, r and
 * one for the true residual -- which dominate; 5 min(nVec, 8) fine vectors (r and z rounded, s, t, w) and (2 coarseIters + 2) min(nVec, 8)
 * coarse vectors in fp32, half of what the cycle takes in mugiq_hip_mg_solve; 0.6 MB of scalars.  32^4, nKrylov 16, 8 right-hand sides:
 * 59 GB are used, as many as by mugiq_hip_mg_solve (58 GB): the two vectors of the hand-over take what the halved cycle saves.  The growth
 * rule of the workspace is the same. */
int mugiq_hip_mg_solve_mixed(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                             const MugiqHipCloverField *clover, double kappa, const MugiqHipGaugeField *gaugeSloppy,
                             const MugiqHipCloverField *cloverSloppy, const MugiqHipTransfer *transferSloppy,
                             const MugiqHipCoarseOperator *coarseOpSloppy, const MugiqHipMgSolveParam *param, int *iters_out, double *relres_out,
                             double *history_out, int historyStride, int *hostReads_out, const MugiqHipComm *comm, void *stream);
/* dst_i = src_i, i < nVec, between spinor fields of either precision: the two conversions of the mixed solve as an entry point.  One
 * geometry and field order for all; dst and src each with their own stride and parity offset; no dst overlapping any src.  fp64 -> fp32
 * rounds to nearest even, once; fp32 -> fp64 is exact; equal precisions copy.  Blocks of 8, pads neither read nor written. */
int mugiq_hip_mg_convert_precision(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec, void *stream);
/* dst->V = src->V between two transfers of equal geometry (X, geoBlockSize, nVec, spinBlockSize, and for a coarse -> coarse transfer the
 * colours of its finer side) and either precision, each with its own stride and parity offset: a sloppy hierarchy without a round trip
 * through the host.  One rounding on the store, pads neither read nor written; finest-level and coarse -> coarse transfers alike.
 * Different geometries, a NULL V or overlapping buffers: MUGIQ_HIP_ERROR_INVALID_ARGUMENT, before any device work. */
int mugiq_hip_transfer_convert(const MugiqHipTransfer *dst, const MugiqHipTransfer *src, void *stream);

/* ---- the three-level solve (new; csrc/mg_solve.hip): the K-cycle through the coarsest operator, what the reference's MG_Mugiq runs with
 * n_level 3.  The eight entry points above do not change, in bits or in refusals; they are these with nCoarseLevels = 1.
 *
 * Levels.  Level 0 is the fine lattice with M.  Level l >= 1 carries the explicit operator M_l = coarseOps_h[l-1]; T_l = transfers_h[l]
 * connects level l and l + 1; R_l and P_l are the batched restriction and prolongation (finest-level for l = 0, coarse -> coarse for
 * l >= 1).  L = nCoarseLevels in {1, 2}.
 *   Cyc(A, R, P, S; nuPre, nuPost, omega)(r):  z = 0, s = r;  nuPre MR steps on A;  if S is given: z += P S(R s), s = r - A z (one
 *     application);  nuPost MR steps;  returns z.  Word for word the K of mugiq_hip_mg_solve, with the same elisions of copies.
 *   GCRflex(A, C, b, n):  x = 0, r = b; for k < n:  p = C(r), q = A p, then the step of GCRfix (classical Gram-Schmidt in one pass, the
 *     nu = 0 guard, alpha = <q, r> / nu taken in the orthogonalising pass).  Returns x.
 *   K_1   = Cyc(M_1, R_1, P_1, GCRfix(M_2, ., params[1].coarseIters); params[1])        (S absent for params[1].coarseIters = 0)
 *   K^(3) = Cyc(M,   R_0, P_0, GCRflex(M_1, K_1, ., params[0].coarseIters); params[0])  (S absent for params[0].coarseIters = 0)
 * With L = 1 the level-1 solve is GCRfix(M_1, ., params[0].coarseIters) and the cycle IS K.  The outer solve is that of
 * mugiq_hip_mg_solve with p = K^(3)(r).
 * Parameters.  params_h[0] is the whole MugiqHipMgSolveParam of the two-grid calls: tol, maxIter and nKrylov of the outer solve and the
 * cycle on level 0.  Of params_h[1] only nuPre, nuPost, omega and coarseIters are used; the rest is range-checked and ignored.
 * nuPre + nuPost + coarseIters = 0 in params_h[1] would make K_1 = 0 and is MUGIQ_HIP_ERROR_INVALID_ARGUMENT.  params_h[0].coarseIters = 0
 * is allowed: levels 1 and 2 are then never touched (but still checked).  The struct defaults are NOT tuned for level 1.
 * Promises, as for the two-grid calls: blocks of 8 right-hand sides with a mask, a converged one is not touched, one solved alone equals
 * the same one in any batch bit for bit, no atomics and fixed summation orders, identical bits, counts and histories from two runs, pads
 * neither read nor written, K^(3)(2^k r) = 2^k K^(3)(r) bit for bit; in fp32 storage every load is widened, sums are fp64 and the store
 * rounds once.  Nothing is read back inside K^(3): hostReads stays max(iters of the block) + 2 per block of 8.
 * Refused before any device work: nCoarseLevels outside 1 .. 2 (MUGIQ_HIP_ERROR_UNSUPPORTED); a process grid or a partitioned axis
 * (UNSUPPORTED); the precision rules of the twin for EVERY object of the hierarchy (mixed precisions inside one hierarchy: UNSUPPORTED in
 * the fp64 calls, INVALID_ARGUMENT in the sloppy and mixed ones); transfers_h[1] not a spinBlockSize 1 transfer on the lattice of
 * coarseOps_h[0] with parity_offset = 2 coarseOps_h[0].nVec nVec stride; coarseOps_h[1] not on the coarse side of transfers_h[1] with its
 * nVec; kappa or hasClover mismatches of either operator; overlapping fields or operators; parameter ranges per level.
 * Work memory (per-stream operator workspace), beyond that of the twin: per right-hand side of a block 3 level-1 vectors (s, t, w of K_1)
 * and 2 params[1].coarseIters + 2 level-2 vectors; the result of K_1 goes straight into the direction slot p_k of level 1.  In all for
 * mugiq_hip_mg_precondition_levels: 3 min(nVec, 8) fine, (2 params[0].coarseIters + 5) min(nVec, 8) level-1 and
 * (2 params[1].coarseIters + 2) min(nVec, 8) level-2 vectors and 0.6 MB of scalars; the solves add the fine vectors of their twins. */
int mugiq_hip_mg_precondition_levels(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                                     const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfers_h,
                                     const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                     const MugiqHipComm *comm, void *stream);
int mugiq_hip_mg_solve_levels(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                              const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfers_h,
                              const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h, int *iters_out,
                              double *relres_out, double *history_out, int historyStride, int *hostReads_out, const MugiqHipComm *comm, void *stream);
/* everything in precision 4, as mugiq_hip_mg_precondition_sloppy */
int mugiq_hip_mg_precondition_sloppy_levels(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                                            const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfers_h,
                                            const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                            const MugiqHipComm *comm, void *stream);
/* fp64 fields and outer GCR, the whole hierarchy in precision 4, as mugiq_hip_mg_solve_mixed */
int mugiq_hip_mg_solve_mixed_levels(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                                    const MugiqHipCloverField *clover, double kappa, const MugiqHipGaugeField *gaugeSloppy,
                                    const MugiqHipCloverField *cloverSloppy, const MugiqHipTransfer *transfersSloppy_h,
                                    const MugiqHipCoarseOperator *coarseOpsSloppy_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                    int *iters_out, double *relres_out, double *history_out, int historyStride, int *hostReads_out,
                                    const MugiqHipComm *comm, void *stream);

/* ---- the deflated coarsest solve (new; csrc/mg_deflate.hip): the coarsest level of the MG solve seeded with the lowest eigenvectors of
 * M_L^dag M_L, the vectors mugiq_hip_coarse_eigensolve computes on that level for the loops.  What QUDA's multigrid does with
 * mg_param.use_eig_solver on its coarsest level (tests/loop.cpp:474, 813-820) and coarse_guess (tests/loop.cpp:592).  M_L is the explicit
 * operator of the LAST coarse level given to a call, coarseOps_h[nCoarseLevels - 1]; only that level is deflated, the levels above it
 * keep their flexible GCR.  It pays where the coarsest solve is the weak link of the cycle.
 *
 * The space.  w_n: orthonormal, the nEv lowest eigenvectors of M_L^dag M_L; u_n = M_L w_n / sigma_n with sigma_n = ||M_L w_n|| > 0, so
 * that (sigma_n, u_n, w_n) are the lowest singular triplets of M_L.  mugiq_hip_coarse_deflation_build makes U and sigma from W.
 *   GCRdefl(A, D, b, n):  c_n = <u_n, b>;  x0 = sum_n w_n (c_n / sigma_n);  r0 = b - sum_n u_n c_n  (n ascending in both);
 *                         x = x0 + GCRfix(A, r0, n): the recurrence of mugiq_hip_mg_solve started from (x0, r0), its first update
 *                         accumulating into x instead of assigning it.
 * r0 is NOT recomputed as b - A x0: with exact triplets the two are equal, with approximate ones they differ by the order of the
 * eigensolver's residual, and the outer GCR is flexible -- a preconditioner that is slightly off costs iterations, never accuracy.  So the
 * projection applies no operator (x0 = W Theta^-1 W^dag A^dag b, r0 = b - A x0 would apply two).
 * With a space, the last-level solve GCRfix(M_L, ., coarseIters) of every cycle above becomes GCRdefl(M_L, D, ., coarseIters); nothing else
 * changes.  Where that level is never reached (params_h[0].coarseIters = 0, or params_h[1].coarseIters = 0 with two coarse levels) the space
 * is checked but not read.
 *
 * The projection is two passes (csrc/mg_deflate.hip): the overlaps c[n][r] over element chunks x groups of eigenvectors, U read once per
 * block of <= 8 right-hand sides, per-chunk partial sums added in ascending chunk order by a small kernel that also forms c_n / sigma_n;
 * then one pass, one element per lane, that reads w_n and u_n once and writes both x0 and r0.  fp64 arithmetic in either storage, one
 * rounding on the store, no atomics; the bits of c[n][r] depend on u_n, b_r and the field geometry alone -- not on nEv, nVec, the mask or
 * the place in the batch.  Pads are neither read nor written; an inactive right-hand side is not touched. */
typedef struct MugiqHipCoarseDeflation_s {
  int nEv;                      /* 1 .. 1024, no multiple of anything */
  const MugiqHipCoarseField *W; /* [nEv] w_n: lowest eigenvectors of M_L^dag M_L (what mugiq_hip_coarse_eigensolve returns for MdagM) */
  const MugiqHipCoarseField *U; /* [nEv] u_n = M_L w_n / sigma_n, unit norm */
  const double *sigma;          /* [nEv], host, sigma_n = ||M_L w_n|| > 0 */
} MugiqHipCoarseDeflation;

/* U_n = M_L W_n / sigma_n and sigma_n = ||M_L W_n|| for n < nEv: the application in blocks of 8, the norm by a fixed-order fp64 sum, one
 * blocking read per block.  W, U and op of one precision (4 | 8); any strides, one for all W and one for all U; no U may overlap a W or
 * another U.  A sigma_n that is 0 or not finite: MUGIQ_HIP_ERROR_INVALID_ARGUMENT with sigma_h filled (u_n is then left unscaled).  A
 * single domain only.  Work memory: 64 KB of scalars in the per-stream operator workspace. */
int mugiq_hip_coarse_deflation_build(const MugiqHipCoarseField *U_h, double *sigma_h, const MugiqHipCoarseField *W_h, int nEv,
                                     const MugiqHipCoarseOperator *op, const MugiqHipComm *comm, void *stream);
/* The projection alone: x0_i and r0_i of GCRdefl for b_i, i < nVec, in blocks of 8 -- the coarse guess, and the kernels without a solve.
 * x0, r0 and b: 3 nVec distinct fields of the space's lattice, n_vec and precision, of one stride and parity offset; none may overlap a
 * w_n or u_n.  A vector alone equals the same vector in any batch, bit for bit.  Work memory as below. */
int mugiq_hip_coarse_deflate(const MugiqHipCoarseField *x0_h, const MugiqHipCoarseField *r0_h, const MugiqHipCoarseField *b_h, int nVec,
                             const MugiqHipCoarseDeflation *space, const MugiqHipComm *comm, void *stream);
/* The four *_levels entry points with a space: their argument lists plus `deflation` after params_h.  deflation == NULL IS the twin: the
 * same code path, the same bits.  The space must live on the lattice and n_vec of coarseOps_h[nCoarseLevels - 1], in that hierarchy's
 * precision (the mixed solve: the sloppy one, 4).
 * Promises.  Every promise of the twins carries over: blocks of 8 right-hand sides with a mask, a converged one is not touched, one solved
 * alone equals the same one in any batch bit for bit, two runs give identical bits, counts and histories, pads neither read nor written,
 * fp64 sums in fp32 storage with one rounding on the store, K(2^k r) = 2^k K(r) bit for bit (the projection is linear and its scalars
 * scale exactly).  Nothing is read back inside the cycle: hostReads stays max(iters of the block) + 2 per block of 8.
 * Refused before any device work, beyond the refusals of the twins: nEv outside 1 .. 1024; NULL members; a w_n or u_n that differs from
 * the last operator in lattice, n_vec or precision, or within its set in stride or parity offset; w_n or u_n overlapping each other or
 * the call's fields; a sigma_n that is not positive and finite.
 * Work memory, beyond that of the twin, in a buffer of its own carved from the per-stream operator workspace (not the Krylov scalars):
 * sigma and the two body tables (3 nEv words), the coefficients c and c / sigma ([nEv][8] complex each) and the chunk partials
 * ([nChunks][nEv][8] complex): 8 nEv (35 + 16 nChunks) bytes, nChunks = ceil(E / max(2048, 64 ceil(E / 16384))) <= 256 for E complex
 * elements per vector (196 608 elements and 200 vectors: 96 chunks, 2.5 MB). */
int mugiq_hip_mg_precondition_levels_deflated(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec, const MugiqHipGaugeField *gauge,
                                              const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfers_h,
                                              const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                              const MugiqHipCoarseDeflation *deflation, const MugiqHipComm *comm, void *stream);
int mugiq_hip_mg_solve_levels_deflated(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                                       const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer *transfers_h,
                                       const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                       const MugiqHipCoarseDeflation *deflation, int *iters_out, double *relres_out, double *history_out,
                                       int historyStride, int *hostReads_out, const MugiqHipComm *comm, void *stream);
int mugiq_hip_mg_precondition_sloppy_levels_deflated(const MugiqHipSpinorField *z_h, const MugiqHipSpinorField *r_h, int nVec,
                                                     const MugiqHipGaugeField *gauge, const MugiqHipCloverField *clover, double kappa,
                                                     const MugiqHipTransfer *transfers_h, const MugiqHipCoarseOperator *coarseOps_h, int nCoarseLevels,
                                                     const MugiqHipMgSolveParam *params_h, const MugiqHipCoarseDeflation *deflation,
                                                     const MugiqHipComm *comm, void *stream);
int mugiq_hip_mg_solve_mixed_levels_deflated(const MugiqHipSpinorField *x_h, const MugiqHipSpinorField *b_h, int nVec, const MugiqHipGaugeField *gauge,
                                             const MugiqHipCloverField *clover, double kappa, const MugiqHipGaugeField *gaugeSloppy,
                                             const MugiqHipCloverField *cloverSloppy, const MugiqHipTransfer *transfersSloppy_h,
                                             const MugiqHipCoarseOperator *coarseOpsSloppy_h, int nCoarseLevels, const MugiqHipMgSolveParam *params_h,
                                             const MugiqHipCoarseDeflation *deflation, int *iters_out, double *relres_out, double *history_out,
                                             int historyStride, int *hostReads_out, const MugiqHipComm *comm, void *stream);

/* ---- MG setup (new; csrc/mg_setup.hip): what QUDA's newMultigridQuda does before MG_Mugiq / Eigsolve_Mugiq see a transfer
 * (tests/loop.cpp:347-365: setup_inv, setup_maxiter, setup_tol, num_setup_iter, n_block_ortho) -- from a gauge field to V and M_c.
 *
 * Block orthonormalisation, in place on V (QUDA's BlockOrthogonalize).  For every aggregate and every coarse spin S (finest level: the
 * chirality s / spinBlockSize) let B be the m x n_vec block of V whose rows are all (x in the aggregate; s with s / spinBlockSize = S; c):
 * m = 6 aggVol on the finest level, m = nColor aggVol on a coarse -> coarse level.  For pass < nPasses, for j = 0 .. n_vec - 1:
 *   c_i = <q_i, b_j> for all i < j, taken from the un-updated b_j (classical Gram-Schmidt, one reduction round per 16 columns: the idiom
 *   of GCRfix above);  b_j -= sum_i c_i q_i;  nu_j = ||b_j||;  q_j = b_j / nu_j;  nu_j = 0: the column is stored as exact zeros and counted.
 * The result is the Q of the thin QR with positive real diagonal, columns in their given order.  nPasses: 1 .. 4 (QUDA's n_block_ortho
 * defaults to 1; one classical pass loses orthogonality as kappa(B)^2 eps, the second restores it: "twice is enough").
 * Arithmetic and sums in fp64 for either storage precision of V, one rounding on the store of a column (every pass stores; the finished
 * columns q_i are read as stored).  No atomics; the order of every sum is fixed by the level geometry alone (rows in the lexicographic
 * order of the LOCAL site coordinates in the aggregate, x fastest, spin-colour rows outermost): the call is bitwise reproducible, and the
 * bits of a block depend neither on the other blocks nor on the lattice the aggregate sits in.  Pads are never read or written.
 * info (may be NULL): minPivotRatio = the minimum over blocks and columns of the FIRST pass's nu_j / ||b_j as given|| (0 for a zero
 * column), zeroColumns = the columns stored as zeros; one host read at the end.  minPivotRatio < rankTol: MUGIQ_HIP_ERROR_INVALID_ARGUMENT
 * after filling V and info all the same; rankTol = 0 never fails.  A NaN is not turned into a zero column: it spreads through its own
 * column and the later columns of its block, which come back as NaN, minPivotRatio is NaN (which fails every rankTol > 0), and
 * zeroColumns does not count it.
 * transfer: either layout MugiqHipTransfer describes, checked before any device work as mugiq_hip_prolongate_batched (spinBlockSize 2)
 * or mugiq_hip_prolongate_coarse_batched (spinBlockSize 1) check it.  The colours of the finer side of a coarse -> coarse V are not in
 * the descriptor: they are taken from parity_offset = 2 nColor n_vec stride, which must hold exactly.  n_vec <= m;  a column of m rows
 * in fp64 and the row table (24 m bytes) must fit the LDS of a workgroup (m <= 6 600 or so; MUGIQ_HIP_ERROR_UNSUPPORTED beyond). */
typedef struct MugiqHipBlockOrthoInfo_s {
  double minPivotRatio;
  int zeroColumns;
} MugiqHipBlockOrthoInfo;
int mugiq_hip_block_orthonormalize(const MugiqHipTransfer *transfer /* V is written */, int nPasses, double rankTol,
                                   MugiqHipBlockOrthoInfo *info, void *stream);
/* out[0] = max over the blocks of max_ij |(B^dag B - 1)_ij|, by the same fixed-order fp64 sums: the check a user runs on a V they were
 * handed (in the spirit of computeEvals and the plaquette).  One host read. */
int mugiq_hip_transfer_orthonormality(const MugiqHipTransfer *transfer, double *out, void *stream);
/* V(x; s, c, j) = vecs_h[j](x; s, c) for all j < nVec = transfer->nVec, and its inverse for one column.  transfer: a finest-level one;
 * the vectors: its lattice, either precision (converted on the way if it differs from V's), FLOAT2 | FLOAT4, any stride; pads of
 * neither side are read or written. */
int mugiq_hip_transfer_set_vectors(const MugiqHipTransfer *transfer /* V is written */, const MugiqHipSpinorField *vecs_h, int nVec, void *stream);
int mugiq_hip_transfer_get_vector(const MugiqHipSpinorField *vec, const MugiqHipTransfer *transfer, int j, void *stream);
/* The same for a coarse -> coarse transfer (spinBlockSize 1; csrc/coarse_op2.hip): V(x; s, c, j) = vecs_h[j](x; s, c) for coarse vectors
 * on its finer lattice with nColor = the colours of that side (parity_offset = 2 nColor n_vec stride, exactly), and its inverse for one
 * column.  Either precision on each side (converted on the way), any strides (one for all vectors); pads are neither read nor written. */
int mugiq_hip_transfer_set_coarse_vectors(const MugiqHipTransfer *transfer /* V is written */, const MugiqHipCoarseField *vecs_h, int nVec, void *stream);
int mugiq_hip_transfer_get_coarse_vector(const MugiqHipCoarseField *vec, const MugiqHipTransfer *transfer, int j, void *stream);

/* The setup driver: host code over the entry points above and below.  start_h: nVec = transfer->nVec fp64 start vectors the caller
 * fills (e.g. seeded Gaussian noise; there is no device RNG).  Null vector j is QUDA's "M x = 0 from a random guess":
 *   b = M start_j;  e = mugiq_hip_wilson_clover_solve(b) stopped at setupMaxIter or setupTol (MUGIQ_HIP_ERROR_NOT_CONVERGED is expected
 *   and absorbed);  v_j = start_j - e,
 * in blocks of 8.  Then V = pack(v), mugiq_hip_block_orthonormalize(nBlockOrtho, rankTol) and, if coarseOp is given,
 * mugiq_hip_compute_coarse_operator.  refineCycles > 0 (QUDA's num_setup_iter > 1; needs coarseOp, MUGIQ_HIP_ERROR_INVALID_ARGUMENT
 * otherwise, and fp64): each cycle v_j -= mugiq_hip_mg_solve(M v_j) with the current V and M_c, stopped after refineIters outer
 * iterations (defaults of mugiq_hip_mg_solve_param_default otherwise; tol = setupTol, nKrylov = refineIters), then repack,
 * re-orthonormalise and rebuild M_c.  A rank failure of the orthonormalisation ends the setup with its status, V and info filled.
 * The finest level only (a second one: mugiq_hip_compute_coarse_operator_coarse) and one domain: a comm with more than one rank or a partitioned axis is
 * MUGIQ_HIP_ERROR_UNSUPPORTED before any device work.  The start vectors are only read.  Work memory: nVec + 16 fine fp64 vectors,
 * allocated for the call and freed, plus what the calls it makes take from the per-stream workspace.
 * Defaults: setupMaxIter 500 and setupTol 5e-6 mirror tests/loop.cpp:349-350;  nBlockOrtho 2, rankTol 1e-8, refineCycles 0 and
 * refineIters 4 are first guesses, NOT tuned. */
typedef struct MugiqHipMgSetupParam_s {
  int setupMaxIter;  /* >= 0 CG iterations per null vector */
  double setupTol;   /* > 0: tolerance of the CG (and of the refinement solves) */
  int nBlockOrtho;   /* 1 .. 4 passes of the block orthonormalisation */
  double rankTol;    /* 0 .. 1: see mugiq_hip_block_orthonormalize */
  int refineCycles;  /* 0 .. 16 */
  int refineIters;   /* 1 .. 16 outer iterations of a refinement solve */
} MugiqHipMgSetupParam;
typedef struct MugiqHipMgSetupInfo_s {
  int cgIters[64];        /* CG iterations of null vector j */
  double minPivotRatio;   /* of the last orthonormalisation */
  int zeroColumns;
  double orthonormality;  /* mugiq_hip_transfer_orthonormality of the final V */
  int hostReads;          /* blocking reads the call COUNTED: one per orthonormalisation, one for the final check, and those
                             mugiq_hip_mg_solve reports for the refinement solves.  The CG's reads are not in it */
  int cgHostReadsEstimate; /* NOT counted: mugiq_hip_wilson_clover_solve reports no reads, so this is what its source makes for the
                             iteration counts above -- 2 max(cgIters) + 3 per block of 8 -- and goes stale if that solver changes */
} MugiqHipMgSetupInfo;
int mugiq_hip_mg_setup_param_default(MugiqHipMgSetupParam *p);
int mugiq_hip_mg_setup(const MugiqHipTransfer *transfer /* V is written */, MugiqHipCoarseOperator *coarseOp /* may be NULL */,
                       const MugiqHipSpinorField *start_h, int nVec, const MugiqHipGaugeField *gauge,
                       const MugiqHipCloverField *clover /* may be NULL */, double kappa, const MugiqHipMgSetupParam *p,
                       MugiqHipMgSetupInfo *info, const MugiqHipComm *comm /* NULL: one domain */, void *stream);

/* ---- the coarse-grid eigensolver (new; csrc/coarse_eig.hip, csrc/dense_herm.cpp): Eigsolve_Mugiq::computeEvecs
 * (lib/eigsolve_mugiq.cpp:278-287) in the computeCoarse branch (:27-33), where the reference hands mg_env->diracCoarse to QUDA's
 * eigensolver with the QudaEigParam members tests/eigensolve.cpp:251-289 fills from the command line (nConv, nKr, tol, max_restarts,
 * use_norm_op, use_poly_acc, poly_deg, a_min, a_max): in production the normal operator MdagM, the smallest real part of the spectrum,
 * Chebyshev acceleration on.  Here: a Chebyshev-filtered block subspace iteration, shaped by
 * mugiq_hip_coarse_apply, which reads the matrices once per 8 vectors.  tests/coarse_eig_ref.py restates it in numpy, step for step.
 *
 * Definitions.  A = MdagM | MMdag of the coarse operator (Hermitian, positive); Q a basis of m = nKr coarse vectors; <a, b> = sum conj(a) b
 * in fp64 fixed-order sums.
 *   Bounds.  aMax > 0 is taken as given; aMax <= 0: 20 power steps of A on the first 8 start vectors, each vector normalised after each
 *     step, then aMax = 1.1 max_j <x_j, A x_j> from one more application.  After every Rayleigh-Ritz step, if the largest Ritz value
 *     exceeds aMax: aMax = 1.1 x that value (a Ritz value never exceeds lambda_max, so this only repairs an underestimate).  The first time
 *     this happens to a GIVEN aMax, the bound has been shown wrong, and a Ritz value repairs it only as far as the basis reaches (a filter
 *     whose aMax is still below lambda_max amplifies the top of the spectrum): the power estimate above then runs once after all, 21
 *     block applications and 21 host reads, and aMax is the larger of the two.
 *   orth(Y): nOrtho rounds of Cholesky QR -- G = Y^dag Y (mugiq_hip_coarse_gram), G = R^dag R and R^-1 on the host, Y <- Y R^-1
 *     (mugiq_hip_coarse_rotate).  A pivot <= rankTol max diag G ends the call with MUGIQ_HIP_ERROR_INVALID_ARGUMENT, outputs and info
 *     filled from the basis as it stands (the convention of mugiq_hip_block_orthonormalize).
 *   Rayleigh-Ritz: W = A Q in blocks of 8, H = Q^dag W Hermitised as (H + H^dag) / 2, H = Z Theta Z^dag with Theta ascending
 *     (mugiq_hip_hermitian_eigh), Q <- Q Z and W <- W Z (A is not applied again), r_i = ||W_i - theta_i Q_i||.  Pair i is converged when
 *     r_i <= tol aMax; nLocked = the largest multiple of 8 such that every i < nLocked is converged.
 *   Filter: for the columns i >= nLocked in blocks of 8, Q_i <- T_d(A) Q_i by QUDA's unscaled recurrence with a = aMin, b = aMax,
 *     d1 = 2 / (b - a), d2 = -(b + a) / (b - a), d = polyDeg:  t_0 = q,  t_1 = d1 A q + d2 q,  t_{k+1} = 2 (d1 A t_k + d2 t_k) - t_{k-1}.
 *     aMin > 0 is fixed (the reference's eig_amin); aMin <= 0 is adaptive: before each filter, the largest Ritz value of the previous
 *     Rayleigh-Ritz step.  Locked columns are not filtered; they stay in Q for orth and Rayleigh-Ritz.  A non-finite Gram diagonal after
 *     a filter is MUGIQ_HIP_ERROR_HIP with a message, not an abort.
 *   Driver: Q = orth(start), Rayleigh-Ritz; then filter, orth, Rayleigh-Ritz, iters++ until the first nConv pairs are converged or
 *     iters = maxIter (MUGIQ_HIP_ERROR_NOT_CONVERGED, all outputs filled, as mugiq_hip_mg_solve does).  Returned: the first nConv columns,
 *     theta, r and sigma_i = sqrt(theta_i).
 * The 20 power steps (QUDA: 100), tol, polyDeg, nOrtho and rankTol are first guesses, NOT tuned; the 1.1 is QUDA's. */

/* G_h[i*mB + j] = <a_i, b_j> (complex, row-major, HOST memory: one blocking read per call) for mA x mB coarse vectors of one lattice and
 * n_vec, precision 8 (4: MUGIQ_HIP_ERROR_UNSUPPORTED), any stride (one for all a, one for all b; pads are not read), a comm of more than
 * one rank or with a partitioned axis MUGIQ_HIP_ERROR_UNSUPPORTED.  A tall-skinny complex GEMM on v_mfma_f64_16x16x4_f64; the vector is
 * cut into chunks of 4096 complex elements, the partial of a chunk is written and the chunks are added in ascending order by a second
 * kernel: no atomics.  The bits of G[i][j] depend on a_i, b_j and the field geometry alone -- not on mA, mB or where i and j stand in
 * the batch.  (G[j][i] of a = b is the conjugate of G[i][j] only to rounding: the imaginary part adds its two products in another order.)
 * Work memory (per-stream workspace): (chunks + 1) mA mB complex. */
int mugiq_hip_coarse_gram(double *G_h, const MugiqHipCoarseField *a_h, int mA, const MugiqHipCoarseField *b_h, int mB, const MugiqHipComm *comm,
                          void *stream);
/* out_j = sum_i in_i Z[i][j], i < mIn, j < mOut; Z_h[i*mOut + j] complex, row-major, on the host, copied by the call.  Out of place: an
 * out overlapping an in or another out is MUGIQ_HIP_ERROR_INVALID_ARGUMENT.  Fields as above, one stride for all in and one for all out;
 * pads are neither read nor written.  The same instruction; the sum over i runs in ascending order, four to an instruction, whatever
 * mOut.  An in_i with Z[i][j] = 0 still enters as 0 x in_i: a NaN or Inf there reaches every output.
 * There is no grid twin of this call: a rotation is local to a rank (every rank rotates its block with the same Z), so the grid solver
 * calls the kernel as it is; this entry keeps refusing a partitioned comm, like mugiq_hip_coarse_gram. */
int mugiq_hip_coarse_rotate(const MugiqHipCoarseField *out_h, int mOut, const MugiqHipCoarseField *in_h, int mIn, const double *Z_h,
                            const MugiqHipComm *comm, void *stream);
/* Host-side dense algebra, no device and no LAPACK behind it; matrices are row-major n x n complex (re, im interleaved), n <= 512.
 * eigh: (H + H^dag) / 2 = Z diag(theta) Z^dag, theta ascending, column j of Z the eigenvector of theta_j -- Householder
 *   tridiagonalisation, implicit-shift QL; a non-finite H is MUGIQ_HIP_ERROR_INVALID_ARGUMENT.
 * cholesky_upper: G = R^dag R, R upper triangular with a positive diagonal, from the upper triangle of G.  The first pivot <= rankTol max
 *   diag G, or not finite, is MUGIQ_HIP_ERROR_INVALID_ARGUMENT with *badPivot = its column and *pivot its value (either may be NULL;
 *   *badPivot = -1 on success): reported, never a NaN in R.
 * upper_triangular_inverse: Rinv = R^-1 (upper triangular); a zero or non-finite diagonal entry is MUGIQ_HIP_ERROR_INVALID_ARGUMENT. */
int mugiq_hip_hermitian_eigh(int n, const double *H, double *theta, double *Z);
int mugiq_hip_cholesky_upper(int n, const double *G, double *R, double rankTol, int *badPivot, double *pivot);
int mugiq_hip_upper_triangular_inverse(int n, const double *R, double *Rinv);

typedef struct MugiqHipCoarseEigParam_s {
  int nConv;      /* eig_nConv: 1 <= nConv < nKr */
  int nKr;        /* eig_nKr: a multiple of 8, <= min(512, dimension of the coarse space) */
  double tol;     /* > 0: pair i is converged when r_i <= tol aMax */
  int maxIter;    /* eig_max_restarts: >= 0 filter / orth / Rayleigh-Ritz rounds */
  int polyDeg;    /* eig_poly_deg: >= 1 */
  double aMin;    /* eig_amin; <= 0: adaptive */
  double aMax;    /* eig_amax; <= 0: estimated */
  int nOrtho;     /* 1 .. 3 rounds of Cholesky QR */
  double rankTol; /* 0 .. 1 */
} MugiqHipCoarseEigParam;
typedef struct MugiqHipCoarseEigInfo_s {
  int iters;               /* filter / orth / Rayleigh-Ritz rounds made */
  int nConverged;          /* of the first nConv pairs */
  int opBlocks;            /* applications of A to a block of (at most) 8 vectors */
  double aMaxUsed;         /* the upper bound at the end (estimated or given, then repaired) */
  double aMinLast;         /* the lower bound of the last filter (the given aMin if none ran) */
  double orthonormality;   /* max |E^dag E - 1| of the returned vectors, from one last Gram matrix */
  int hostReads;           /* blocking reads, COUNTED by the call: one per Gram matrix and one per set of residual norms */
  double hostDenseSeconds; /* wall time of the host's eigendecompositions, Cholesky factors and inverses */
} MugiqHipCoarseEigInfo;
/* The members are those tests/eigensolve.cpp:251-289 fills from QUDA's flags; it fixes no values.  nConv 200 is the N_ev of this
 * project's flagship workload, nKr 256 the next multiple of 8 with a quarter to spare; maxIter 100, tol 1e-10, polyDeg 20, aMin 0
 * (adaptive), aMax 0 (estimated), nOrtho 2, rankTol 1e-14: first guesses, NOT tuned. */
int mugiq_hip_coarse_eig_param_default(MugiqHipCoarseEigParam *param);
/* The solver above.  evecs_h[nConv] (written), start_h[nKr] (only read; the caller fills them, e.g. with seeded Gaussian noise: there is
 * no device RNG, as in mugiq_hip_mg_setup): coarse fields of the operator's lattice and n_vec, any stride (one for all evecs, one for all
 * start), no overlaps.  op: an operator of precision 8; opType MdagM | MMdag.  theta_h, residual_h, sigma_h: [nConv].
 * Refusals, each before any device work: parameters out of range (MUGIQ_HIP_ERROR_INVALID_ARGUMENT); a comm of more than one rank or
 * with a partitioned axis (MUGIQ_HIP_ERROR_UNSUPPORTED, as for the coarse operator); opType M | Mdag | H (MUGIQ_HIP_ERROR_UNSUPPORTED);
 * precision 4 in the operator or a field (MUGIQ_HIP_ERROR_UNSUPPORTED); geometry mismatches, nKr above the dimension 4 n_vec volumeCB,
 * overlaps (MUGIQ_HIP_ERROR_INVALID_ARGUMENT).
 * Work memory: three bases of nKr packed vectors plus 24 vectors (and nKr (chunks + 2) doubles), allocated for the call and freed -- a
 * failed allocation is MUGIQ_HIP_ERROR_HIP -- plus what mugiq_hip_coarse_apply, mugiq_hip_coarse_gram and mugiq_hip_coarse_rotate take
 * from the per-stream arenas.  No atomics: two runs give identical bits, counts and info, apart from the seconds. */
int mugiq_hip_coarse_eigensolve(const MugiqHipCoarseField *evecs_h, const MugiqHipCoarseField *start_h, const MugiqHipCoarseOperator *op,
                                int opType, const MugiqHipCoarseEigParam *param, double *theta_h, double *residual_h, double *sigma_h,
                                MugiqHipCoarseEigInfo *info, const MugiqHipComm *comm, void *stream);

/* ---- the coarse eigensolver on a process grid (new; csrc/coarse_eig.hip; tests/coarse_eig_grid_ref.py restates it rank by rank).
 * The solver touches the lattice in three places: the application of A, the Gram matrices and the residual sums.  On a grid A is applied
 * by mugiq_hip_coarse_apply_grid's internals (faces exchanged per launch), and every Gram matrix and every vector of residual sums is
 * added over the ranks in the fixed order of the eigenpair check (reduce_space, gather_time, rank-ordered sum, bcast: the same bits on
 * every rank).  The rotations and the recurrence are local to a rank; the dense host algebra runs on every rank on identical input, so
 * convergence, locking, the aMax repair, every count and every return status are identical on all ranks, and nothing is broadcast beyond
 * those sums.  On ONE rank with axes forced (MugiqHipComm.partitioned) nothing is summed and the applications are the bits of
 * mugiq_hip_coarse_apply: the call gives the bits of mugiq_hip_coarse_eigensolve.  On more ranks the Gram sums are added in another
 * order than on one domain (per rank first), so values agree to rounding, not bit for bit.
 *
 * The Chebyshev step of the filter writes the send faces of the next application (chebyshev_step_pack_kernel: the element of a site on
 * the low or high face of a partitioned axis is stored a second time, into that face's send buffer, in the layout of the face pack:
 * [vector][parity][row][face index]), for the steps k < polyDeg of a block; the first application of a block, Rayleigh-Ritz and the
 * power estimate pack with the pack kernel.  MUGIQ_HIP_EIG_PACK_IN_STEP=0 (read once per call) keeps the plain step kernel and separate
 * packs everywhere; both settings give the same bits. */
typedef struct MugiqHipCoarseEigGridInfo_s {
  int exchanges;    /* face exchanges issued (one per kernel launch of the operator: 2 per block application on a partitioned comm) */
  int rankSums;     /* sums over the ranks made (0 on one rank: there is nothing to add) */
  int packLaunches; /* launches of the face pack kernel made for the solver's applications */
  int stepPacked;   /* exchanges whose send faces were written by the recurrence kernel */
} MugiqHipCoarseEigGridInfo;
/* mugiq_hip_coarse_gram for a rank of a process grid; collective.  The local Gram matrix, by the same two kernels, is added over the ranks:
 * every rank gets the same bits.  comm is required (NULL: MUGIQ_HIP_ERROR_INVALID_ARGUMENT), with reduce_space, gather_time and bcast
 * where it has more than one rank.  On a comm of one rank the call is mugiq_hip_coarse_gram, bit for bit. */
int mugiq_hip_coarse_gram_grid(double *G_h, const MugiqHipCoarseField *a_h, int mA, const MugiqHipCoarseField *b_h, int mB,
                               const MugiqHipComm *comm, void *stream);
/* mugiq_hip_coarse_eigensolve for a rank of a process grid; collective.  op and halo: from mugiq_hip_compute_coarse_operator_grid;
 * evecs_h, start_h: the rank's local blocks.  nKr is checked against the global dimension, 4 n_vec volumeCB x ranks.  info is filled as
 * by the single-domain call (hostReads keeps its meaning and its formula), gridInfo as above.  Checks, each before any device work:
 * comm or gridInfo NULL; those of the grid calls (sendrecv NULL on a partitioned comm; a sum callback NULL with more than one rank;
 * halo NULL on a partitioned comm, of another operator, or not built for a partitioned axis); those of mugiq_hip_coarse_eigensolve.
 * With nothing partitioned (one rank, no forced axis) halo may be NULL and the call runs the existing solver: the same bits. */
int mugiq_hip_coarse_eigensolve_grid(const MugiqHipCoarseField *evecs_h, const MugiqHipCoarseField *start_h, const MugiqHipCoarseOperator *op,
                                     const MugiqHipCoarseHalo *halo, int opType, const MugiqHipCoarseEigParam *param, double *theta_h,
                                     double *residual_h, double *sigma_h, MugiqHipCoarseEigInfo *info, MugiqHipCoarseEigGridInfo *gridInfo,
                                     const MugiqHipComm *comm, void *stream);

/* What Displace asks of QUDA's ColorSpinorField for its auxiliary vector (lib/displace.cpp:26-30: ColorSpinorField::Create
 * with QUDA_ZERO_FIELD_CREATE and setPrecision(coarsePrec_); :42,:50-51: operator=; :59: blas::zero), for hosts that do not
 * manage device memory themselves.  alloc: geometry, order, stride of `like`, `precision` (0 = like's), zeroed; ghost zones
 * (zeroed) for the dims with ghostDims[d] != 0 (NULL = none).  copy: same precision / order / geometry required. */
int mugiq_hip_alloc_spinor_like(MugiqHipSpinorField *out, const MugiqHipSpinorField *like, int precision, const int ghostDims[4]);
int mugiq_hip_free_spinor(MugiqHipSpinorField *f);
int mugiq_hip_copy_spinor(const MugiqHipSpinorField *dst, const MugiqHipSpinorField *src, void *stream);
int mugiq_hip_zero_spinor(const MugiqHipSpinorField *f, void *stream);

/* MugiqLoopParam (include/mugiq.h:28-47) with C arrays instead of std::vector/std::string.
 * gauge: the reference hands over host QDP-ordered links + a QudaGaugeParam and lets Displace build the
 * border-extended device field (lib/displace.cpp:104-134); here the extended device field is the input
 * (mugiq_amd builds it; see GaugeField).  May be NULL when doNonLocal == 0. */
typedef struct MugiqHipLoopParam_s {
  int Nmom;
  const int *momMatrix; /* [Nmom][3] */
  int FTSign;           /* LoopFTSign: -1 | +1 */
  int calcType;         /* MUGIQ_HIP_LOOP_CALC_TYPE_* */
  int writeMomSpaceHDF5;
  int writePosSpaceHDF5;
  int doMomProj;
  int doNonLocal;
  int nDispEntries;              /* disp_str.size() */
  const char *const *disp_entry; /* e.g. "+z:1,8" */
  const char *const *disp_str;   /* e.g. "+z" */
  const int *disp_start;
  const int *disp_stop;
  const char *fname_mom_h5;
  const char *fname_pos_h5;
  const MugiqHipGaugeField *gauge;
  int loopPrecision;             /* not in the reference: 0 = the eigenvectors' precision; 8 with fp32 eigenvectors = mixed
                                    precision (fp32 storage, fp64 accumulation, loop buffers, FT and output) */
} MugiqHipLoopParam;

/* Loop_Mugiq::LoopComputeParam + the element counts of allocateDataMemory
 * (include/loop_mugiq.h:141-271, lib/loop_mugiq.cpp:101-109) */
typedef struct MugiqHipLoopInfo_s {
  int nDispEntries, nLoop, nData, Nmom, precision, field_order, loopPrecision;
  int localL[4], totalL[4];
  int locT, totT;
  long long locV4, locV3, totV3;
  long long nElemPosLocPerLoop, nElemMomLocPerLoop, nElemMomTotPerLoop;
  long long nElemPosLoc, nElemMomLoc, nElemMomTot, nElemPhMat;
} MugiqHipLoopInfo;

typedef struct MugiqHipLoop_s MugiqHipLoop;

/* Loop_Mugiq::Loop_Mugiq(loopParams, eigsolve)  lib/loop_mugiq.cpp:6-59: takes what the class reads from
 * Eigsolve_Mugiq as a friend -- eVecs[0..nEv) and eVals_sigma[0..nEv) (lib/loop_mugiq.cpp:442,479) -- sets up
 * LoopComputeParam, allocates the data buffers, creates the phase matrix.  comm may be NULL (single process).
 * The descriptors are copied; the eigenvector memory stays the caller's.
 * Links need not be unitary (anisotropy-rescaled, smeared and not re-projected, fp32 links in fp64 storage).  At create and at the
 * start of every OPT compute a pre-pass over the gauge field (one thread per line, per direction with entries: about 0.13 ms per
 * direction at 48x48x24x24, and one host synchronisation) measures how far the axial gauge of each direction is from unitary; the
 * flags are summed over all ranks through the comm callbacks, so every rank decides alike.  Directions above the tolerance take the
 * vector tiles (one-sided) or the step-by-step sequence (two-sided) instead of the matrix-pipe tile. */
int mugiq_hip_loop_create(MugiqHipLoop **loop, const MugiqHipLoopParam *param, const MugiqHipSpinorField *eVecs_h,
                          const double *eVals_sigma_h, int nEv, const MugiqHipComm *comm, void *stream);
/* Two-sided loops (new): sum_r (1/sigma_r) vL_r^dag(x) G [D^k vR_r](x) for every entry, with separate left (eVecsL_h) and right
 * (eVecsR_h, the displaced set) vectors of the same geometry, precision and order; fine-level vectors only.  Output pipeline (G -> g5 G
 * reorder, momentum projection, HDF5 tree) as for mugiq_hip_loop_create.  No entry is reflected from its opposite-sign partner
 * (mugiq_hip_loop_entry_derived_from is -1 for all), only the right set travels in halos, and halo face layers are packed by
 * their own kernels.  For M^-1 ~ sum_r w_r phi_r xi_r^dag pass eVecsR = phi_r, eVecsL = g5 xi_r, sigma_r = 1 / w_r. */
int mugiq_hip_loop_create_two_sided(MugiqHipLoop **loop, const MugiqHipLoopParam *param, const MugiqHipSpinorField *eVecsL_h,
                                    const MugiqHipSpinorField *eVecsR_h, const double *sigma_h, int n, const MugiqHipComm *comm,
                                    void *stream);
/* The same with eigsolve->useMGenv && eigsolve->computeCoarse (lib/loop_mugiq.cpp:42,482; configs[4]): the
 * eigenvectors are COARSE fields and are prolonged with `transfer` (mugiq_hip_prolongate_batched) -- once, not once
 * per displacement entry; without displacement entries the ultra-local loop runs through
 * mugiq_hip_prolongate_contract_batched and the fine vectors are never stored.  fineFieldOrder must be 2
 * ("Vector prolongation requires fieldOrder = FLOAT2", lib/loop_mugiq.cpp:283). */
int mugiq_hip_loop_create_coarse(MugiqHipLoop **loop, const MugiqHipLoopParam *param,
                                 const MugiqHipCoarseField *coarseEvecs_h, const double *eVals_sigma_h, int nEv,
                                 const MugiqHipTransfer *transfer, int fineFieldOrder, const MugiqHipComm *comm,
                                 void *stream);
/* The same for an MG hierarchy with nCoarseLevels = mg_param.n_level - 1 >= 1 coarse levels (include/mg_mugiq.h:20,30): the
 * eigenvectors live on the COARSEST level; transfers_h[0] is the finest transfer (fine lattice <-> level 1, spinBlockSize 2),
 * transfers_h[l], l >= 1, the one between level l and level l+1 (see mugiq_hip_prolongate_coarse_batched).  Every compute
 * prolongs all eigenvectors level by level (lib/loop_mugiq.cpp:306-314) into temporaries the loop object owns. */
int mugiq_hip_loop_create_coarse_levels(MugiqHipLoop **loop, const MugiqHipLoopParam *param,
                                        const MugiqHipCoarseField *coarsestEvecs_h, const double *eVals_sigma_h, int nEv,
                                        const MugiqHipTransfer *transfers_h, int nCoarseLevels, int fineFieldOrder,
                                        const MugiqHipComm *comm, void *stream);
/* Loop_Mugiq::computeCoarseLoop()  lib/loop_mugiq.cpp:439-525 (position-space loops for the ultra-local case and
 * every displacement entry, then performMomentumProjection :322-434 if doMomProj).  Synchronises `stream`. */
int mugiq_hip_loop_compute(MugiqHipLoop *loop);
int mugiq_hip_loop_get_info(const MugiqHipLoop *loop, MugiqHipLoopInfo *info);
/* slot bookkeeping of entry id: (dir, sign, start, stop, nLoopPerEntry, nLoopOffset) -> out6[6] */
int mugiq_hip_loop_get_entry(const MugiqHipLoop *loop, int id, int out6[6]);
/* After mugiq_hip_loop_compute: the entry that entry `id` was reflected from (see mugiq_hip_reflect_displaced_loop), or
 * -1 if it was computed from the eigenvectors; -2 for a bad handle / index. */
int mugiq_hip_loop_entry_derived_from(const MugiqHipLoop *loop, int id);
/* After mugiq_hip_loop_compute: how entry `id` was produced (one-sided and two-sided loops alike), or -1 for a bad handle / index or
 * before the first compute. */
#define MUGIQ_HIP_ENTRY_KERNEL_REFLECTED 0    /* derived from its opposite-sign partner (position or momentum space) */
#define MUGIQ_HIP_ENTRY_KERNEL_MFMA_COLUMN 1  /* matrix-pipe tile, column tile (mu = y, z, t; csrc/fused_mfma_kernel.h) */
#define MUGIQ_HIP_ENTRY_KERNEL_MFMA_ROW 2     /* matrix-pipe tile, row tile (mu = x) */
#define MUGIQ_HIP_ENTRY_KERNEL_VECTOR_TILE 3  /* LDS-tiled vector kernels (csrc/fused_tile.hip, csrc/fused_tile16.hip) */
#define MUGIQ_HIP_ENTRY_KERNEL_STREAMING 4    /* the streaming fused kernel (csrc/fused.hip) */
#define MUGIQ_HIP_ENTRY_KERNEL_STEPWISE 5     /* one displacement + one contraction per step (BASIC plan and its fallbacks) */
int mugiq_hip_loop_get_entry_kernel(const MugiqHipLoop *loop, int id);
/* After mugiq_hip_loop_compute: the displacement entry whose pass over the eigenvectors also produced the ultra-local loop
 * (mugiq_hip_displaced_loop_contraction_fused_carry), or -1 if the ultra-local loop took a pass of its own. */
int mugiq_hip_loop_ultra_local_carrier(const MugiqHipLoop *loop);
/* After mugiq_hip_loop_compute: the number of posted halos whose face layers were written by the entry that runs first, on its way
 * through the eigenvectors, instead of by mugiq_hip_pack_face_layers beside it (fp64 FLOAT2, first entry along x on the row tile,
 * z / t partitioned; MUGIQ_HIP_PACK_IN_ENTRY=0 switches it off).  0: none; -1: bad handle / nothing computed yet. */
int mugiq_hip_loop_halos_packed_in_entry(const MugiqHipLoop *loop);
/* The plan of a compute (new; host only, no device work): what mugiq_hip_loop_compute does with every displacement entry, through
 * the function the driver itself plans with (csrc/loop_plan.cpp), under the same environment switches.  param as for
 * mugiq_hip_loop_create (param->gauge: precision and R only); eVec: the geometry of the eigenvectors; comm may be NULL, its
 * callbacks are not called; axialOk[mu]: the outcome of the unitarity pre-pass along mu; deviceBytes: the device's total memory.
 * No data pointer is read. */
#define MUGIQ_HIP_LOOP_ROUTE_REFLECTED 0 /* derived from its opposite-sign partner */
#define MUGIQ_HIP_LOOP_ROUTE_STEPWISE 1  /* one displacement + one contraction per step */
#define MUGIQ_HIP_LOOP_ROUTE_FUSED 2     /* the fused displaced contraction */
#define MUGIQ_HIP_LOOP_PLAN_MAX_ENTRIES 64
#define MUGIQ_HIP_LOOP_PLAN_MAX_BUFFERS 512
typedef struct MugiqHipLoopEntryPlan_s {
  int derivedFrom;         /* the entry it is reflected from, or -1 */
  int route;               /* MUGIQ_HIP_LOOP_ROUTE_* */
  int part, high;          /* its direction is partitioned; the face it sends (0 low, 1 high) */
  int kStart, nK;          /* its lengths kStart .. kStart + nK - 1 */
  int tile;                /* the matrix-pipe tile may take it (the pre-pass along its direction passed) */
  int gaugeFromField;      /* its axial gauge is built straight from the gauge field: no path-link fields */
  int nLinkFields;         /* path-link fields W_0 .. W_stop it builds (0 | stop + 1) */
  int buildGaugeFromLinks; /* the driver builds its axial gauge from those fields, once for all its launches */
  int ahead, selfAlias;    /* its halo is posted at the start of the compute; the neighbour is the rank itself and nothing is sent */
  int nBlocks, blockN;     /* the blocks of eigenvectors it is processed (ahead: its halo travels) in */
  int needsMemset;         /* its slots are accumulated into */
  int entryPacksFrom;      /* >= 0: the entry that runs first writes its face layers from this eigenvector on; -1: pack kernels */
  int kernel;              /* MUGIQ_HIP_ENTRY_KERNEL_* that mugiq_hip_loop_get_entry_kernel reports after the compute */
  long long faceBytes, haloBytes, perVecHaloBytes, gaugeBytes;
} MugiqHipLoopEntryPlan;
typedef struct MugiqHipLoopPlan_s {
  int nEntries, nOrder, nPackTargets, nReserve;
  int earlyEntry; /* the entry that runs before the halos are packed, or -2 */
  int carryUltra, momReflect, grouped;
  int order[MUGIQ_HIP_LOOP_PLAN_MAX_ENTRIES + 1];     /* -1: the ultra-local loop */
  int packTargets[MUGIQ_HIP_LOOP_PLAN_MAX_ENTRIES];   /* the posted entries whose face layers earlyEntry writes */
  long long reserve[MUGIQ_HIP_LOOP_PLAN_MAX_BUFFERS]; /* buffers reserved when the loop object is created, in order */
  MugiqHipLoopEntryPlan entry[MUGIQ_HIP_LOOP_PLAN_MAX_ENTRIES];
} MugiqHipLoopPlan;
int mugiq_hip_loop_plan(const MugiqHipLoopParam *param, const MugiqHipSpinorField *eVec, int nEv, int twoSided, int coarseMode,
                        const MugiqHipComm *comm, const int axialOk[4], size_t deviceBytes, MugiqHipLoopPlan *out);
/* The kernel form of one fused displaced entry (new; host only): what mugiq_hip_displaced_loop_contraction_fused* and the loop driver
 * select for it (csrc/fused_form.cpp, the one place that decides), under the same environment switches, and the geometry of its first
 * launch.  ev: the geometry, precision and order of the eigenvectors (no data pointer is read); partitioned: along dispDir;
 * gaugeGiven: the caller holds the axial gauge (the driver: always); loopPrecision 0: that of ev. */
#define MUGIQ_HIP_FUSED_FAMILY_NONE 0        /* two-sided and no matrix-pipe tile: the step-by-step sequence */
#define MUGIQ_HIP_FUSED_FAMILY_MFMA_COLUMN 1 /* matrix-pipe column tile */
#define MUGIQ_HIP_FUSED_FAMILY_MFMA_ROW 2    /* matrix-pipe row tile */
#define MUGIQ_HIP_FUSED_FAMILY_TILE32 3      /* 32-line vector tile (csrc/fused_tile.hip) */
#define MUGIQ_HIP_FUSED_FAMILY_TILE16 4      /* 16-line vector tile (csrc/fused_tile16.hip) */
#define MUGIQ_HIP_FUSED_FAMILY_STREAMING 5   /* streaming kernel (csrc/fused.hip) */
typedef struct MugiqHipFusedForm_s {
  int kernel, family;               /* MUGIQ_HIP_ENTRY_KERNEL_*, MUGIQ_HIP_FUSED_FAMILY_* */
  int slotsPerLaunch, packCapacity; /* displaced slots per launch at most; face-layer targets a mu = x entry can write on its way */
  long long gaugeBytes;             /* its axial gauge (0: no matrix-pipe tile) */
  /* the first launch: its slots, its longest length, and per family (0 where it does not apply) */
  int nSlots, kmax, waves, staged;  /* staged: positions along mu held in LDS */
  int tj, lines;                    /* positions along mu and lines per tile */
  int rowGroups, rows, rowChunk, leftBufElems; /* matrix-pipe: row tile geometry; two-sided left image */
  int ph, glds;                     /* vector tiles: staged global -> LDS; 32-line: bound of positions staged per lane */
  int npc, np, m, phl;              /* 16-line: computed / staged positions, pieces per parity, bound of staging loads per lane */
  long long ldsBytes;
} MugiqHipFusedForm;
int mugiq_hip_fused_form(const MugiqHipSpinorField *ev, int twoSided, int dispDir, const int *kValues, int nK, int partitioned,
                         int gaugeGiven, int loopPrecision, MugiqHipFusedForm *out);
/* Phase timing of a compute (measurement aid; off by default).  When switched on, mugiq_hip_loop_compute brackets each
 * phase with a pair of HIP events on the stream the phase runs on and, after its final synchronisation, reports the
 * device time between them.  Phases of different streams overlap in time (that is the point of the halo stream). */
#define MUGIQ_HIP_PHASE_ULTRA_LOCAL 0          /* the ultra-local slot (lib/loop_mugiq.cpp:501-502 over all eigenvectors) */
#define MUGIQ_HIP_PHASE_ENTRY_FUSED 1          /* a displacement entry computed from the eigenvectors, one domain along its axis */
#define MUGIQ_HIP_PHASE_ENTRY_REFLECTED 2      /* an entry derived from its opposite-sign partner */
#define MUGIQ_HIP_PHASE_ENTRY_STEPWISE 3       /* an entry through the step-by-step sequence (BASIC plan, or length > local extent) */
#define MUGIQ_HIP_PHASE_MOMENTUM_PROJECTION 4  /* reorder + Fourier sums on the device */
#define MUGIQ_HIP_PHASE_HALO_TRANSFER 5        /* eigenvector halo on the halo stream; bytes = what this rank sends */
#define MUGIQ_HIP_PHASE_ENTRY_INTERIOR 6       /* partitioned entry: tiles that need no ghost layers */
#define MUGIQ_HIP_PHASE_ENTRY_BOUNDARY 7       /* partitioned entry: tiles that read the ghost layers */
#define MUGIQ_HIP_PHASE_PROLONGATION 8         /* MG path: coarse -> fine for all eigenvectors */
#define MUGIQ_HIP_PHASE_HALO_PREPARE 9         /* path-link fields + packing of the face layers of one entry; bytes packed */
#define MUGIQ_HIP_PHASE_HALO_WAIT 10           /* compute stream idle until the halo has landed (what the overlap did not hide) */
#define MUGIQ_HIP_PHASE_MOMENTUM_COPY 11       /* dataMom_d -> pinned host */
#define MUGIQ_HIP_PHASE_MOMENTUM_REDUCE 12     /* host: reduce over space ranks, gather over time ranks, broadcast (wall time) */
#define MUGIQ_HIP_PHASE_TOTAL_WALL 13          /* host wall time of the whole mugiq_hip_loop_compute call (always the last phase) */
#define MUGIQ_HIP_PHASE_MOMENTUM_REFLECT 15     /* host: reflected entries derived on the gathered momentum-space array (wall time) */
#define MUGIQ_HIP_PHASE_SCRATCH_ALLOC 14       /* host: hipMalloc of scratch / halo buffers the pool did not hold yet (wall time, bytes) */
#define MUGIQ_HIP_PHASE_AXIAL_CHECK 16         /* OPT plan: the unitarity pre-pass of the axial-gauge tile (kernels, one host read, the cross-rank sum) */
typedef struct MugiqHipLoopPhase_s {
  int kind;     /* MUGIQ_HIP_PHASE_* */
  int entry;    /* displacement entry the phase belongs to, or -1 */
  double ms;    /* device time between the bracketing events (host wall time for kinds 12, 13) */
  double bytes; /* halo / copy phases: bytes moved by this rank; else 0 */
} MugiqHipLoopPhase;
int mugiq_hip_loop_set_profiling(MugiqHipLoop *loop, int on);
/* phases of the last compute, in issue order; returns their number (may exceed max_phases; out may be NULL to ask) */
int mugiq_hip_loop_get_phases(const MugiqHipLoop *loop, MugiqHipLoopPhase *out, int max_phases);
/* dataPos_d: [nLoop][16][V even-odd] complex, device.  dataPos (host) is copied on first request
 * (the reference copies it unconditionally at lib/loop_mugiq.cpp:512).
 * With momentum projection on, the OPT plan derives reflected displacement entries in MOMENTUM space
 * (mugiq_hip_reflect_momentum_space) and leaves their position-space slots out of the compute; the first call of either accessor
 * after such a compute produces them (mugiq_hip_reflect_displaced_loop), so what is returned is always complete.  On a process
 * grid with a reflected entry along a partitioned direction that first call exchanges the slots' boundary layers through
 * comm->sendrecv: every rank must make it.  MUGIQ_HIP_REFLECT_MOM=0 keeps everything in position space inside the compute. */
const void *mugiq_hip_loop_data_pos_d(const MugiqHipLoop *loop);
const void *mugiq_hip_loop_data_pos_h(MugiqHipLoop *loop);
/* dataMom_bcast (host): per time-rank slabs of t + locT*ig + locT*16*iL + locT*16*nLoop*im, concatenated in
 * coord[3] order (lib/loop_mugiq.cpp:415-424).  NULL before compute or without doMomProj. */
const void *mugiq_hip_loop_data_mom_bcast_h(const MugiqHipLoop *loop);
/* Loop_Mugiq::writeLoopsHDF5()  lib/loop_mugiq.cpp:668-693 -> writeLoopsHDF5_Mom :529-656: group tree
 * /mom_%+d_%+d_%+d/disp_0|disp_<+-dir>_<len>/<GammaName>/loop, dataset [totT][2] of native float|double.
 * World rank 0 writes the whole file with serial HDF5 from dataMom_bcast (libhdf5 is bound at run time; override the
 * library with MUGIQ_HIP_HDF5_LIB).  Position-space output is "Not supported yet!" as in the reference (:660-663). */
int mugiq_hip_loop_write_hdf5(MugiqHipLoop *loop);
/* The writer on its own (host only, no GPU needed): dataMom_bcast_h as laid out by performMomentumProjection
 * (lib/loop_mugiq.cpp:415-424); disp_start <= disp_stop already normalised; nLoop = 1 + sum(stop-start+1). */
int mugiq_hip_write_loops_hdf5_mom(const char *filename, const void *dataMom_bcast_h, int precision, int Nmom,
                                   const int *momMatrix, int nDispEntries, const char *const *disp_str,
                                   const int *disp_start, const int *disp_stop, int locT, int totT);
/* mugiq_hip_deflate_low_modes with the eigenvectors, sigma, comm and stream of a one-sided fine-level loop object.
 * MUGIQ_HIP_ERROR_UNSUPPORTED for two-sided and coarse (MG) loop objects. */
int mugiq_hip_loop_deflate(MugiqHipLoop *loop, const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h,
                           int nVec, int gamma5, double *overlaps_h);
/* mugiq_hip_deflate_low_modes_coarse with the coarse eigenvectors, sigma, transfers, comm and stream of a coarse (MG) loop object.
 * MUGIQ_HIP_ERROR_UNSUPPORTED for fine-level and two-sided loop objects. */
int mugiq_hip_loop_deflate_coarse(MugiqHipLoop *loop, const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h,
                                  int nVec, int gamma5, double *overlaps_h);
/* Loop_Mugiq::~Loop_Mugiq */
int mugiq_hip_loop_destroy(MugiqHipLoop *loop);

/* ---- a6 (setup): Displace::createExtendedCudaGaugeField  lib/displace.cpp:70-134 ------------------------------------ */
/* bytes of a pad-0 extended field: volExCB * 36 * 2 parities * sizeof(complex) */
size_t mugiq_hip_extended_gauge_bytes(const int X[4], const int R[4], int precision);
/* Allocate (zeroed, pad 0) and describe the extended field for local dims X and border R -- gParamEx of
 * lib/displace.cpp:104-124 -- for hosts that do not manage device memory themselves; release with
 * mugiq_hip_free_extended_gauge. */
int mugiq_hip_alloc_extended_gauge(MugiqHipGaugeField *gauge, const int X[4], const int R[4], int precision);
int mugiq_hip_free_extended_gauge(MugiqHipGaugeField *gauge);
/* Fill gauge->data (device, caller-allocated, descriptor complete) from the host links of the LOCAL lattice in
 * QDP order, qdpLinks_h[dir][(parity*V/2 + x_cb)*18 + (row*3+col)*2 + re/im] of cpuPrecision (4|8)
 * (loopParams.gauge[4], tests/loop.cpp:88,106,902-918), then fill the R-deep borders: neighbour slabs through
 * comm->sendrecv for partitioned dims (edges/corners included, like exchangeExtendedGhost), periodic wrap otherwise. */
int mugiq_hip_create_extended_gauge(const MugiqHipGaugeField *gauge, const void *const qdpLinks_h[4], int cpuPrecision,
                                    const MugiqHipComm *comm, void *stream);

/* ---- stout smearing of the extended gauge field, its border refresh and the plaquette (csrc/smear.hip; new) ---------------------------
 * Displaced loops run on a second gauge field (--loop-gauge-filename, tests/loop.cpp:902-918), in production a smeared copy of the
 * configuration; the reference prints the plaquette of what it loaded (tests/loop.cpp:895-898).  One stout step (Morningstar and
 * Peardon, hep-lat/0311018) of a link U_mu(x) that is smeared, S the set of smeared directions:
 *   C_mu(x)  = sum_{nu in S, nu != mu} [ U_nu(x) U_mu(x+nu) U_nu^dag(x+mu)  +  U_nu^dag(x-nu) U_mu(x-nu) U_nu(x-nu+mu) ]
 *   Omega    = rho C_mu(x) U_mu^dag(x)
 *   Q        = (i/2) (Omega^dag - Omega) - (i/6) tr(Omega^dag - Omega) 1              (Hermitian, traceless)
 *   U'_mu(x) = exp(iQ) U_mu(x)
 * smearDims = 3: S = {x, y, z}; the spatial links are smeared with spatial staples and the t links are copied unchanged.
 * smearDims = 4: S = all four directions, every link is smeared.  U^dag is the conjugate transpose of the link as stored, as everywhere
 * else in the library.  exp(iQ) = f0 + f1 Q + f2 Q^2 analytically (Cayley-Hamilton) from c0 = det Q and c1 = tr Q^2 / 2 in the
 * (u, w, xi0(w)) form of that paper, with the series of xi0 for small w and the symmetry c0 -> -c0.  Q = 0 (rho = 0, pure-gauge links, a
 * constant abelian field) has c1 = 0, where the closed form is 0/0: for c1 <= 1e-14 (Q^3/6 below 1e-21) the series 1 + iQ - Q^2/2 is
 * taken, which is exact to rounding there and gives U' = U without a NaN.  Every step reads the field of the step before: smearing is out of place, with a
 * ping-pong between two fields.  fp64 arithmetic whatever the storage, rounded once per step on the store.
 *
 * Plaquette:
 *   P_mn(x)  = Re tr [ U_m(x) U_n(x+m) U_m^dag(x+n) U_n^dag(x) ] / 3
 *   spatial  = mean over the local sites of all ranks and the planes xy, xz, yz
 *   temporal = mean over the local sites of all ranks and the planes xt, yt, zt
 *   plaq[0]  = (spatial + temporal) / 2,  plaq[1] = spatial,  plaq[2] = temporal
 * This is the normalisation ASSUMED for QUDA's plaqQuda (1 for unit links); QUDA is not available to this project, so it has not
 * been compared against it.
 *
 * Links are addressed in the extended field as mugiq_hip_compute_clover addresses them: x +- nu across a face comes from the border
 * where R >= 1 and wraps where R = 0, x - nu + mu from the edge regions.  A partitioned dimension (comm) with R[d] = 0, or without
 * comm->sendrecv, is MUGIQ_HIP_ERROR_INVALID_ARGUMENT for all three calls, as are a NULL descriptor or data, a precision other than
 * 4 | 8, odd local dims and an odd sum of the borders; all of it is checked before any device work. */
/* Refresh the R-deep borders of a device-resident field from its interior: the device counterpart of the border half of
 * mugiq_hip_create_extended_gauge (the reference's exchangeExtendedGhost, lib/displace.cpp:127).  One dimension after the other, later
 * ones carrying the borders of earlier ones (edges and corners); a dimension that is not partitioned is wrapped on the device, a
 * partitioned one goes pack kernel -> comm->sendrecv -> unpack kernel.  The result equals, bit for bit, what
 * mugiq_hip_create_extended_gauge builds from the same interior.  Pads are not written. */
int mugiq_hip_exchange_extended_gauge(const MugiqHipGaugeField *gauge, const MugiqHipComm *comm, void *stream);
/* nSteps stout steps of `in` into `out` (same X, R and precision; strides may differ; the buffers must not overlap:
 * MUGIQ_HIP_ERROR_INVALID_ARGUMENT otherwise, and for nSteps < 0, smearDims not 3 | 4, rho not finite).  The borders of `in` must be
 * valid (mugiq_hip_create_extended_gauge or mugiq_hip_exchange_extended_gauge).  One kernel per step and a border refresh after every
 * step: `out` ends complete, borders included; `in` is never written.  nSteps >= 2 allocates one temporary field inside the call and
 * frees it (set-up-time code); nSteps = 0 copies `in` to `out`.  Pads are not written. */
int mugiq_hip_stout_smear(const MugiqHipGaugeField *out, const MugiqHipGaugeField *in, double rho, int nSteps, int smearDims,
                          const MugiqHipComm *comm, void *stream);
/* plaq_h[3] = {mean, spatial, temporal} of the definition above, summed over the ranks of comm (NULL: one process; otherwise
 * reduce_space, gather_time and bcast must be set when size > 1).  One local site per lane, a fixed-order fp64 reduction: bitwise
 * reproducible, and identical on every rank.  Blocks the host. */
int mugiq_hip_plaquette(const MugiqHipGaugeField *gauge, double plaq_h[3], const MugiqHipComm *comm, void *stream);

/* ---- user syntax (tests/loop.cpp:607-705) -------------------------------------------------------------------------- */
/* Parse "+z:1,8;-x:3;+y:2,5".  Returns the number of entries (<= max_entries) or a negative MugiqHipStatus.
 * disp_str_out: max_entries x 4 chars ("+z\0"); start/stop as in setLoopParam. */
int mugiq_hip_parse_displace_entry_string(const char *entry_string, int max_entries, char *disp_str_out,
                                          int *disp_start_out, int *disp_stop_out);
/* Displace::WhichDisplaceFlag/Dir/Sign (lib/displace.cpp:137-202): "+x".."-t" -> dir, sign; non-zero if unparsable */
int mugiq_hip_parse_displacement(const char *disp_str, int *dir_out, int *sign_out);

#ifdef __cplusplus
}
#endif
#endif /* MUGIQ_HIP_H */
