// mugiq_hip_operators.hpp -- C++ host-side mirror of MuGiq's operator API over the C ABI of libmugiq_hip.so.
//
// Same template names, argument order and meaning as the reference's wrappers
// (lib/contract_wrappers.cu; declared at include/loop_mugiq.h:280-311 and include/displace.h:109-111), with
// MugiqHipSpinorField / MugiqHipGaugeField standing in for quda::ColorSpinorField / cudaGaugeField, plus the
// enums (include/enum_mugiq.h), MugiqLoopParam (include/mugiq.h:28-47) and the public surface of
// Loop_Mugiq<Float,order> (include/loop_mugiq.h:123-134).  Where the reference aborts through errorQuda, these
// throw mugiq_hip::Error carrying the same message.  Header-only; link with -lmugiq_hip.
//
// Inside a MuGiq/QUDA build include mugiq_hip_quda_adapter.hpp instead: it defines MUGIQ_HIP_NO_REFERENCE_ENUMS (MuGiq's own
// enum_mugiq.h provides the enums) and MUGIQ_HIP_WITH_QUDA, and produces the descriptors from QUDA fields.
#ifndef MUGIQ_HIP_OPERATORS_HPP
#define MUGIQ_HIP_OPERATORS_HPP

#include <array>
#include <climits>
#include <complex>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "mugiq_hip.h"

#ifndef MUGIQ_HIP_NO_REFERENCE_ENUMS
#include "mugiq_hip_enums.hpp"  // MuGiq's enums (inside a MuGiq build its own enum_mugiq.h provides them)
#endif

namespace mugiq_hip {

constexpr int FLOAT2_FIELD_ORDER = MUGIQ_HIP_FLOAT2_FIELD_ORDER;  // QUDA_FLOAT2_FIELD_ORDER
constexpr int FLOAT4_FIELD_ORDER = MUGIQ_HIP_FLOAT4_FIELD_ORDER;  // QUDA_FLOAT4_FIELD_ORDER

struct Error : std::runtime_error {
  int status;
  Error(int st, const std::string &msg) : std::runtime_error(msg), status(st) {}
};
inline void check(int status) {
  if (status != 0) throw Error(status, mugiq_hip_last_error());
}

using ColorSpinorField = MugiqHipSpinorField;
using GaugeField = MugiqHipGaugeField;

template <typename Float> constexpr int precisionOf() {
  static_assert(sizeof(Float) == 4 || sizeof(Float) == 8, "Float must be float or double");
  return (int)sizeof(Float);
}
template <typename Float, int order> inline void checkField(const ColorSpinorField *f, const char *who) {
  if (f->precision != precisionOf<Float>() || f->field_order != order)
    throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, std::string(who) + ": field precision/order does not match the template arguments");
}

// lib/contract_wrappers.cu:6-19, 26-43
template <typename Float> inline void copyGammaCoeffStructToSymbol() { check(mugiq_hip_copy_gamma_coeff_to_symbol(precisionOf<Float>())); }
template <typename Float> inline void copyGammaMapStructToSymbol() { check(mugiq_hip_copy_gamma_map_to_symbol(precisionOf<Float>())); }

// lib/contract_wrappers.cu:50-77 (commCoord replaces QUDA's comm_coord(); NULL = single process)
template <typename Float>
inline void createPhaseMatrixGPU(std::complex<Float> *phaseMatrix_d, const int *momMatrix_h, long long locV3, int Nmom, int FTSign,
                                 const int localL[], const int totalL[], const int commCoord[] = nullptr, void *stream = nullptr) {
  check(mugiq_hip_create_phase_matrix(phaseMatrix_d, momMatrix_h, locV3, Nmom, FTSign, localL, totalL, commCoord,
                                      precisionOf<Float>(), stream));
}

// lib/contract_wrappers.cu:88-115
template <typename Float, int fieldOrder>
inline void performLoopContraction(std::complex<Float> *loopData_d, ColorSpinorField *eVecL, ColorSpinorField *eVecR, Float sigma,
                                   void *stream = nullptr) {
  checkField<Float, fieldOrder>(eVecL, "performLoopContraction");
  checkField<Float, fieldOrder>(eVecR, "performLoopContraction");
  check(mugiq_hip_perform_loop_contraction(loopData_d, eVecL, eVecR, (double)sigma, stream));
}

// the eigenvector loop of lib/loop_mugiq.cpp:478-503 in one launch (new)
template <typename Float, int fieldOrder>
inline void performLoopContractionBatched(std::complex<Float> *loopData_d, const std::vector<ColorSpinorField> &eVecL,
                                          const std::vector<ColorSpinorField> &eVecR, const std::vector<double> &sigma,
                                          void *stream = nullptr) {
  if (eVecL.empty() || eVecL.size() != eVecR.size() || eVecL.size() != sigma.size())
    throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "performLoopContractionBatched: size mismatch");
  checkField<Float, fieldOrder>(&eVecL[0], "performLoopContractionBatched");
  check(mugiq_hip_perform_loop_contraction_batched(loopData_d, eVecL.data(), eVecR.data(), sigma.data(), (int)eVecL.size(), stream));
}

// dst_r <- dst_r - sum_n v_n sigma_n^-1 v_n^dag G src_r, G = g5 | 1 (mugiq_hip_deflate_low_modes; new).  sigma empty: sigma = 1;
// overlaps != nullptr receives c_nr as [nEv][nVec] (resized).  dst may be src.
inline void deflateLowModes(const std::vector<ColorSpinorField> &dst, const std::vector<ColorSpinorField> &src,
                            const std::vector<ColorSpinorField> &eVecs, const std::vector<double> &sigma = {}, bool gamma5 = true,
                            std::vector<std::complex<double>> *overlaps = nullptr, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (src.empty() || dst.size() != src.size() || eVecs.empty() || (!sigma.empty() && sigma.size() != eVecs.size()))
    throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "deflateLowModes: size mismatch");
  if (overlaps) overlaps->assign(eVecs.size() * src.size(), std::complex<double>(0.0, 0.0));
  check(mugiq_hip_deflate_low_modes(dst.data(), src.data(), (int)src.size(), eVecs.data(), sigma.empty() ? nullptr : sigma.data(),
                                    (int)eVecs.size(), gamma5 ? 1 : 0, overlaps ? reinterpret_cast<double *>(overlaps->data()) : nullptr,
                                    comm, stream));
}

// QUDA Transfer::R = P^dag for all vectors in one launch (mugiq_hip_restrict_batched; new): coarse_n = V^dag G fine_n per aggregate
inline void restrictVecs(const std::vector<MugiqHipCoarseField> &coarse, const std::vector<ColorSpinorField> &fine, const MugiqHipTransfer &transfer,
                         bool gamma5 = false, void *stream = nullptr) {
  if (fine.empty() || coarse.size() != fine.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "restrictVecs: size mismatch");
  check(mugiq_hip_restrict_batched(coarse.data(), fine.data(), (int)fine.size(), &transfer, gamma5 ? 1 : 0, stream));
}
// ... and for one coarse -> coarse level (mugiq_hip_restrict_coarse_batched), the adjoint of transfer[lev-1]->P
inline void restrictCoarseVecs(const std::vector<MugiqHipCoarseField> &coarser, const std::vector<MugiqHipCoarseField> &finer,
                               const MugiqHipTransfer &transfer, void *stream = nullptr) {
  if (finer.empty() || coarser.size() != finer.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "restrictCoarseVecs: size mismatch");
  check(mugiq_hip_restrict_coarse_batched(coarser.data(), finer.data(), (int)finer.size(), &transfer, stream));
}
// deflateLowModes for eigenvectors on the coarsest MG level, v_n = P w_n never stored (mugiq_hip_deflate_low_modes_coarse; new);
// transfers: finest first
inline void deflateLowModesCoarse(const std::vector<ColorSpinorField> &dst, const std::vector<ColorSpinorField> &src,
                                  const std::vector<MugiqHipCoarseField> &coarseEvecs, const std::vector<MugiqHipTransfer> &transfers,
                                  const std::vector<double> &sigma = {}, bool gamma5 = true, std::vector<std::complex<double>> *overlaps = nullptr,
                                  const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (src.empty() || dst.size() != src.size() || coarseEvecs.empty() || transfers.empty() || (!sigma.empty() && sigma.size() != coarseEvecs.size()))
    throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "deflateLowModesCoarse: size mismatch");
  if (overlaps) overlaps->assign(coarseEvecs.size() * src.size(), std::complex<double>(0.0, 0.0));
  check(mugiq_hip_deflate_low_modes_coarse(dst.data(), src.data(), (int)src.size(), coarseEvecs.data(), sigma.empty() ? nullptr : sigma.data(),
                                           (int)coarseEvecs.size(), transfers.data(), (int)transfers.size(), gamma5 ? 1 : 0,
                                           overlaps ? reinterpret_cast<double *>(overlaps->data()) : nullptr, comm, stream));
}

// ---- the Wilson operator and what Eigsolve_Mugiq does with it (csrc/wilson.hip; new) -------------------------------------------
// MuGiqEigOperator of include/enum_mugiq.h:22-25 comes from the enums header; H = g5 M is this library's extension
constexpr int EIG_OPERATOR_H = MUGIQ_HIP_EIG_OPERATOR_H;
// dst_i = scale * A src_i (mugiq_hip_wilson_apply): stands in for (*mat)(w, v) of lib/eigsolve_mugiq.cpp:301
inline void wilsonApply(const std::vector<ColorSpinorField> &dst, const std::vector<ColorSpinorField> &src, const GaugeField &gauge, double kappa,
                        int opType = MUGIQ_HIP_EIG_OPERATOR_M, double scale = 1.0, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (src.empty() || dst.size() != src.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "wilsonApply: size mismatch");
  check(mugiq_hip_wilson_apply(dst.data(), src.data(), (int)src.size(), &gauge, kappa, opType, scale, comm, stream));
}
// Eigsolve_Mugiq::computeEvals, lib/eigsolve_mugiq.cpp:289-315 (sigma: sqrt(Re lambda) for MdagM / MMdag, Re lambda for H, empty otherwise)
inline void computeEvals(const std::vector<ColorSpinorField> &eVecs, const GaugeField &gauge, double kappa, int opType, bool massNormalization,
                         std::vector<std::complex<double>> &lambda, std::vector<double> &residual, std::vector<double> &sigma,
                         const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (eVecs.empty()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "computeEvals: no eigenvectors");
  lambda.assign(eVecs.size(), std::complex<double>(0.0, 0.0));
  residual.assign(eVecs.size(), 0.0);
  sigma.assign(eVecs.size(), 0.0);
  check(mugiq_hip_compute_evals(eVecs.data(), (int)eVecs.size(), &gauge, kappa, opType, massNormalization ? 1 : 0,
                                reinterpret_cast<double *>(lambda.data()), residual.data(), sigma.data(), comm, stream));
  if (opType == MUGIQ_HIP_EIG_OPERATOR_M || opType == MUGIQ_HIP_EIG_OPERATOR_MDAG) sigma.clear();
}
// computeEvals for the computeCoarse branch (lib/eigsolve_mugiq.cpp:27-33; mugiq_hip_compute_evals_coarse; new): coarse eigenvectors, the
// Galerkin operator R M P through `transfers` (finest first); clover NULL: the unimproved operator
inline void computeEvalsCoarse(const std::vector<MugiqHipCoarseField> &coarseEvecs, const std::vector<MugiqHipTransfer> &transfers,
                               const GaugeField &gauge, const MugiqHipCloverField *clover, double kappa, int opType, bool massNormalization,
                               std::vector<std::complex<double>> &lambda, std::vector<double> &residual, std::vector<double> &sigma,
                               const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (coarseEvecs.empty() || transfers.empty()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "computeEvalsCoarse: no eigenvectors / transfers");
  lambda.assign(coarseEvecs.size(), std::complex<double>(0.0, 0.0));
  residual.assign(coarseEvecs.size(), 0.0);
  sigma.assign(coarseEvecs.size(), 0.0);
  check(mugiq_hip_compute_evals_coarse(coarseEvecs.data(), (int)coarseEvecs.size(), transfers.data(), (int)transfers.size(), &gauge, clover, kappa,
                                       opType, massNormalization ? 1 : 0, reinterpret_cast<double *>(lambda.data()), residual.data(), sigma.data(),
                                       comm, stream));
  if (opType == MUGIQ_HIP_EIG_OPERATOR_M || opType == MUGIQ_HIP_EIG_OPERATOR_MDAG) sigma.clear();
}
// ---- the explicit Galerkin coarse operator (MugiqHipCoarseOperator; csrc/coarse_op.hip, csrc/coarse_op2.hip; new): one domain -----------
// Owns the nine matrices per coarse site of a transfer (any level)
class CoarseOperator {
public:
  CoarseOperator(const int Xc[4], int nVec, int precision) { check(mugiq_hip_alloc_coarse_operator(&op_, Xc, nVec, precision)); }
  ~CoarseOperator() { mugiq_hip_free_coarse_operator(&op_); }
  CoarseOperator(const CoarseOperator &) = delete;
  CoarseOperator &operator=(const CoarseOperator &) = delete;
  MugiqHipCoarseOperator *desc() { return &op_; }
  const MugiqHipCoarseOperator *desc() const { return &op_; }

private:
  MugiqHipCoarseOperator op_{};
};
// Xd and Y+-_mu of every coarse site from V, the links and the clover term (NULL: Wilson), kappa folded in (mugiq_hip_compute_coarse_operator)
inline void computeCoarseOperator(CoarseOperator &op, const MugiqHipTransfer &transfer, const GaugeField &gauge, const MugiqHipCloverField *clover,
                                  double kappa, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  check(mugiq_hip_compute_coarse_operator(op.desc(), &transfer, &gauge, clover, kappa, comm, stream));
}
// The operator of a coarse -> coarse transfer from the operator of its finer lattice (mugiq_hip_compute_coarse_operator_coarse): the
// coarsest level of a three-level hierarchy, in the same CoarseOperator; kappa and hasClover are inherited
inline void computeCoarseOperatorCoarse(CoarseOperator &op, const MugiqHipTransfer &transfer, const CoarseOperator &finerOp,
                                        const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  check(mugiq_hip_compute_coarse_operator_coarse(op.desc(), &transfer, finerOp.desc(), comm, stream));
}
// V(x; s, c, j) = vecs[j](x; s, c) of a coarse -> coarse transfer, and one column back (mugiq_hip_transfer_set_coarse_vectors / _get_coarse_vector)
inline void setCoarseVectors(const MugiqHipTransfer &transfer, const std::vector<MugiqHipCoarseField> &vecs, void *stream = nullptr) {
  check(mugiq_hip_transfer_set_coarse_vectors(&transfer, vecs.data(), (int)vecs.size(), stream));
}
inline void getCoarseVector(const MugiqHipCoarseField &vec, const MugiqHipTransfer &transfer, int j, void *stream = nullptr) {
  check(mugiq_hip_transfer_get_coarse_vector(&vec, &transfer, j, stream));
}
// dst_i = scale * A_c src_i on the coarse grid (mugiq_hip_coarse_apply)
inline void coarseApply(const std::vector<MugiqHipCoarseField> &dst, const std::vector<MugiqHipCoarseField> &src, const CoarseOperator &op,
                        int opType = MUGIQ_HIP_EIG_OPERATOR_M, double scale = 1.0, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (src.empty() || dst.size() != src.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "coarseApply: size mismatch");
  check(mugiq_hip_coarse_apply(dst.data(), src.data(), (int)src.size(), op.desc(), opType, scale, comm, stream));
}
// 16, 32 or 64: the output components per workgroup coarseApply takes for nVec vectors on this operator (mugiq_hip_coarse_apply_outputs; host only)
inline int coarseApplyForm(const MugiqHipCoarseOperator &op, int nVec) {
  const int out = mugiq_hip_coarse_apply_outputs(&op, nVec);
  if (out == 0) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, mugiq_hip_last_error());
  return out;
}
// computeEvalsCoarse on the explicit operator (mugiq_hip_compute_evals_coarse_operator): no pass over the fine lattice
inline void computeEvalsCoarse(const std::vector<MugiqHipCoarseField> &coarseEvecs, const CoarseOperator &coarseOp, int opType, bool massNormalization,
                               std::vector<std::complex<double>> &lambda, std::vector<double> &residual, std::vector<double> &sigma,
                               const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (coarseEvecs.empty()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "computeEvalsCoarse: no eigenvectors");
  lambda.assign(coarseEvecs.size(), std::complex<double>(0.0, 0.0));
  residual.assign(coarseEvecs.size(), 0.0);
  sigma.assign(coarseEvecs.size(), 0.0);
  check(mugiq_hip_compute_evals_coarse_operator(coarseEvecs.data(), (int)coarseEvecs.size(), coarseOp.desc(), opType, massNormalization ? 1 : 0,
                                                reinterpret_cast<double *>(lambda.data()), residual.data(), sigma.data(), comm, stream));
  if (opType == MUGIQ_HIP_EIG_OPERATOR_M || opType == MUGIQ_HIP_EIG_OPERATOR_MDAG) sigma.clear();
}
// ---- ... on a process grid (mugiq_hip_compute_coarse_operator_grid, mugiq_hip_coarse_apply_grid, mugiq_hip_compute_evals_coarse_operator_grid;
// new): the same three names with the operator's MugiqHipCoarseHalo (mugiq_hip_alloc_coarse_halo / mugiq_hip_free_coarse_halo) behind the
// operator; collective, comm required.  Compile-checked only (tests/test_coarse_op_grid_cpu.py): the C++ test program does not run them
inline void computeCoarseOperator(CoarseOperator &op, const MugiqHipCoarseHalo &halo, const MugiqHipTransfer &transfer, const GaugeField &gauge,
                                  const MugiqHipCloverField *clover, double kappa, const MugiqHipComm *comm, void *stream = nullptr) {
  check(mugiq_hip_compute_coarse_operator_grid(op.desc(), &halo, &transfer, &gauge, clover, kappa, comm, stream));
}
inline void coarseApply(const std::vector<MugiqHipCoarseField> &dst, const std::vector<MugiqHipCoarseField> &src, const CoarseOperator &op,
                        const MugiqHipCoarseHalo &halo, int opType, double scale, const MugiqHipComm *comm, void *stream = nullptr) {
  if (src.empty() || dst.size() != src.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "coarseApply: size mismatch");
  check(mugiq_hip_coarse_apply_grid(dst.data(), src.data(), (int)src.size(), op.desc(), &halo, opType, scale, comm, stream));
}
inline void computeEvalsCoarse(const std::vector<MugiqHipCoarseField> &coarseEvecs, const CoarseOperator &coarseOp, const MugiqHipCoarseHalo &halo,
                               int opType, bool massNormalization, std::vector<std::complex<double>> &lambda, std::vector<double> &residual,
                               std::vector<double> &sigma, const MugiqHipComm *comm, void *stream = nullptr) {
  if (coarseEvecs.empty()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "computeEvalsCoarse: no eigenvectors");
  lambda.assign(coarseEvecs.size(), std::complex<double>(0.0, 0.0));
  residual.assign(coarseEvecs.size(), 0.0);
  sigma.assign(coarseEvecs.size(), 0.0);
  check(mugiq_hip_compute_evals_coarse_operator_grid(coarseEvecs.data(), (int)coarseEvecs.size(), coarseOp.desc(), &halo, opType,
                                                     massNormalization ? 1 : 0, reinterpret_cast<double *>(lambda.data()), residual.data(),
                                                     sigma.data(), comm, stream));
  if (opType == MUGIQ_HIP_EIG_OPERATOR_M || opType == MUGIQ_HIP_EIG_OPERATOR_MDAG) sigma.clear();
}
// Eigsolve_Mugiq::projectVector, lib/eigsolve_mugiq.cpp:340-348
inline void projectVector(ColorSpinorField &out, ColorSpinorField &in, const std::vector<ColorSpinorField> &eVecs, const MugiqHipComm *comm = nullptr,
                          void *stream = nullptr) {
  if (eVecs.empty()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "projectVector: no eigenvectors");
  check(mugiq_hip_project_vector(&out, &in, eVecs.data(), (int)eVecs.size(), comm, stream));
}
// ---- the two-grid preconditioned GCR (csrc/mg_solve.hip; new) ----
// MugiqHipMgSolveParam with the defaults of mugiq_hip_mg_solve_param_default (first guesses, not tuned)
struct MgSolveParam : MugiqHipMgSolveParam {
  MgSolveParam() { check(mugiq_hip_mg_solve_param_default(this)); }
};
namespace detail {
static_assert(sizeof(MgSolveParam) == sizeof(MugiqHipMgSolveParam), "std::vector<MgSolveParam> is handed over as an array of the C struct");
inline int mgLevels(const std::vector<MugiqHipTransfer> &transfers, const std::vector<MugiqHipCoarseOperator> &coarseOps, const std::vector<MgSolveParam> &params,
                    const char *who) {
  if (transfers.empty() || transfers.size() != coarseOps.size() || transfers.size() != params.size())
    throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, std::string(who) + ": one transfer, coarse operator and MgSolveParam per coarse level");
  return (int)transfers.size();
}
// the outputs of a solve before the call: iters and relres sized for n right-hand sides, *stride = max(maxIter, 1); returns the history
// buffer of n * stride entries (empty where no history is asked for)
inline std::vector<double> mgOutputs(size_t n, int maxIter, bool wantHistory, std::vector<int> &iters, std::vector<double> &relres, int *stride) {
  iters.assign(n, 0);
  relres.assign(n, 0.0);
  *stride = maxIter > 0 ? maxIter : 1;
  return std::vector<double>(wantHistory ? n * (size_t)*stride : 0);
}
// and after it: NOT_CONVERGED is the return value false, every other failure throws; history[r] = the iters[r] entries of right-hand side r
inline bool mgHistory(int st, const std::vector<double> &hist, int stride, const std::vector<int> &iters, std::vector<std::vector<double>> *history) {
  if (st != MUGIQ_HIP_ERROR_NOT_CONVERGED) check(st);
  if (history) {
    history->clear();
    for (size_t i = 0; i < iters.size(); i++) history->emplace_back(hist.begin() + i * stride, hist.begin() + i * stride + iters[i]);
  }
  return st == 0;
}
}  // namespace detail
// z_i = K(r_i): one two-grid cycle (mugiq_hip_mg_precondition); clover NULL: the unimproved operator
inline void mgPrecondition(const std::vector<ColorSpinorField> &z, const std::vector<ColorSpinorField> &r, const GaugeField &gauge,
                           const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer &transfer, const CoarseOperator &coarseOp,
                           const MgSolveParam &param = MgSolveParam(), const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (r.empty() || z.size() != r.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgPrecondition: size mismatch");
  check(mugiq_hip_mg_precondition(z.data(), r.data(), (int)r.size(), &gauge, clover, kappa, &transfer, coarseOp.desc(), &param, comm, stream));
}
// x_r = M^-1 b_r by the flexible GCR preconditioned with that cycle (mugiq_hip_mg_solve).  history[r]: the recursive relative residuals of
// right-hand side r; hostReads: the blocking reads of the call.  Returns false where a right-hand side did not reach tol within maxIter
// (every output is filled all the same); every other failure throws.
inline bool mgSolve(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, const GaugeField &gauge,
                    const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer &transfer, const CoarseOperator &coarseOp,
                    const MgSolveParam &param, std::vector<int> &iters, std::vector<double> &relres, std::vector<std::vector<double>> *history = nullptr,
                    int *hostReads = nullptr, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (b.empty() || x.size() != b.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgSolve: size mismatch");
  int stride;
  std::vector<double> hist = detail::mgOutputs(b.size(), param.maxIter, history != nullptr, iters, relres, &stride);
  const int st = mugiq_hip_mg_solve(x.data(), b.data(), (int)b.size(), &gauge, clover, kappa, &transfer, coarseOp.desc(), &param, iters.data(),
                                    relres.data(), history ? hist.data() : nullptr, stride, hostReads, comm, stream);
  return detail::mgHistory(st, hist, stride, iters, history);
}
// ---- on a process grid (mugiq_hip_mg_precondition_grid, mugiq_hip_mg_solve_grid; new): the same two calls for a rank, with the halo of
// the coarse operator (mugiq_hip_compute_coarse_operator_grid) and a comm, which is required.  r needs ghost zones on the partitioned axes
inline void mgPrecondition(const std::vector<ColorSpinorField> &z, const std::vector<ColorSpinorField> &r, const GaugeField &gauge,
                           const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer &transfer, const CoarseOperator &coarseOp,
                           const MugiqHipCoarseHalo &halo, const MgSolveParam &param, const MugiqHipComm *comm, void *stream = nullptr) {
  if (r.empty() || z.size() != r.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgPrecondition: size mismatch");
  check(mugiq_hip_mg_precondition_grid(z.data(), r.data(), (int)r.size(), &gauge, clover, kappa, &transfer, coarseOp.desc(), &halo, &param, comm, stream));
}
inline bool mgSolve(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, const GaugeField &gauge,
                    const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer &transfer, const CoarseOperator &coarseOp,
                    const MugiqHipCoarseHalo &halo, const MgSolveParam &param, std::vector<int> &iters, std::vector<double> &relres,
                    MugiqHipMgSolveGridInfo &gridInfo, const MugiqHipComm *comm, std::vector<std::vector<double>> *history = nullptr,
                    int *hostReads = nullptr, void *stream = nullptr) {
  if (b.empty() || x.size() != b.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgSolve: size mismatch");
  int stride;
  std::vector<double> hist = detail::mgOutputs(b.size(), param.maxIter, history != nullptr, iters, relres, &stride);
  const int st = mugiq_hip_mg_solve_grid(x.data(), b.data(), (int)b.size(), &gauge, clover, kappa, &transfer, coarseOp.desc(), &halo, &param, iters.data(),
                                         relres.data(), history ? hist.data() : nullptr, stride, hostReads, &gridInfo, comm, stream);
  return detail::mgHistory(st, hist, stride, iters, history);
}
// ---- the mixed-precision solve (csrc/mg_solve.hip; new): the cycle in fp32 storage under the fp64 outer GCR ----
// z_i = K(r_i) with z, r, transfer and coarseOp all of precision 4 (mugiq_hip_mg_precondition_sloppy)
inline void mgPreconditionSloppy(const std::vector<ColorSpinorField> &z, const std::vector<ColorSpinorField> &r, const GaugeField &gauge,
                                 const MugiqHipCloverField *clover, double kappa, const MugiqHipTransfer &transfer, const CoarseOperator &coarseOp,
                                 const MgSolveParam &param = MgSolveParam(), const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (r.empty() || z.size() != r.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgPreconditionSloppy: size mismatch");
  check(mugiq_hip_mg_precondition_sloppy(z.data(), r.data(), (int)r.size(), &gauge, clover, kappa, &transfer, coarseOp.desc(), &param, comm, stream));
}
// mgSolve with p = K(r) in fp32 storage on the sloppy hierarchy (mugiq_hip_mg_solve_mixed); x and b stay fp64.  gaugeSloppy and
// cloverSloppy NULL: the cycle reads gauge and clover.  Outputs and the return value as for mgSolve
inline bool mgSolveMixed(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, const GaugeField &gauge,
                         const MugiqHipCloverField *clover, double kappa, const GaugeField *gaugeSloppy, const MugiqHipCloverField *cloverSloppy,
                         const MugiqHipTransfer &transferSloppy, const CoarseOperator &coarseOpSloppy, const MgSolveParam &param, std::vector<int> &iters,
                         std::vector<double> &relres, std::vector<std::vector<double>> *history = nullptr, int *hostReads = nullptr,
                         const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (b.empty() || x.size() != b.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgSolveMixed: size mismatch");
  int stride;
  std::vector<double> hist = detail::mgOutputs(b.size(), param.maxIter, history != nullptr, iters, relres, &stride);
  const int st = mugiq_hip_mg_solve_mixed(x.data(), b.data(), (int)b.size(), &gauge, clover, kappa, gaugeSloppy, cloverSloppy, &transferSloppy,
                                          coarseOpSloppy.desc(), &param, iters.data(), relres.data(), history ? hist.data() : nullptr, stride, hostReads,
                                          comm, stream);
  return detail::mgHistory(st, hist, stride, iters, history);
}
// ---- the three-level solve (csrc/mg_solve.hip; new): the same four calls on a hierarchy, transfers[l] and coarseOps[l] (descriptors, e.g.
// *CoarseOperator::desc()) per coarse level and params[l] per level; one of each is the two-grid call.  params[1]: nuPre, nuPost, omega and
// coarseIters of the level-1 cycle, whose defaults are not tuned ----
inline void mgPrecondition(const std::vector<ColorSpinorField> &z, const std::vector<ColorSpinorField> &r, const GaugeField &gauge,
                           const MugiqHipCloverField *clover, double kappa, const std::vector<MugiqHipTransfer> &transfers,
                           const std::vector<MugiqHipCoarseOperator> &coarseOps, const std::vector<MgSolveParam> &params, const MugiqHipComm *comm = nullptr,
                           void *stream = nullptr) {
  if (r.empty() || z.size() != r.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgPrecondition: size mismatch");
  const int L = detail::mgLevels(transfers, coarseOps, params, "mgPrecondition");
  check(mugiq_hip_mg_precondition_levels(z.data(), r.data(), (int)r.size(), &gauge, clover, kappa, transfers.data(), coarseOps.data(), L, params.data(), comm,
                                         stream));
}
inline void mgPreconditionSloppy(const std::vector<ColorSpinorField> &z, const std::vector<ColorSpinorField> &r, const GaugeField &gauge,
                                 const MugiqHipCloverField *clover, double kappa, const std::vector<MugiqHipTransfer> &transfers,
                                 const std::vector<MugiqHipCoarseOperator> &coarseOps, const std::vector<MgSolveParam> &params,
                                 const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (r.empty() || z.size() != r.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgPreconditionSloppy: size mismatch");
  const int L = detail::mgLevels(transfers, coarseOps, params, "mgPreconditionSloppy");
  check(mugiq_hip_mg_precondition_sloppy_levels(z.data(), r.data(), (int)r.size(), &gauge, clover, kappa, transfers.data(), coarseOps.data(), L, params.data(),
                                                comm, stream));
}
inline bool mgSolve(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, const GaugeField &gauge,
                    const MugiqHipCloverField *clover, double kappa, const std::vector<MugiqHipTransfer> &transfers,
                    const std::vector<MugiqHipCoarseOperator> &coarseOps, const std::vector<MgSolveParam> &params, std::vector<int> &iters,
                    std::vector<double> &relres, std::vector<std::vector<double>> *history = nullptr, int *hostReads = nullptr,
                    const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (b.empty() || x.size() != b.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgSolve: size mismatch");
  const int L = detail::mgLevels(transfers, coarseOps, params, "mgSolve");
  int stride;
  std::vector<double> hist = detail::mgOutputs(b.size(), params[0].maxIter, history != nullptr, iters, relres, &stride);
  const int st = mugiq_hip_mg_solve_levels(x.data(), b.data(), (int)b.size(), &gauge, clover, kappa, transfers.data(), coarseOps.data(), L, params.data(),
                                           iters.data(), relres.data(), history ? hist.data() : nullptr, stride, hostReads, comm, stream);
  return detail::mgHistory(st, hist, stride, iters, history);
}
inline bool mgSolveMixed(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, const GaugeField &gauge,
                         const MugiqHipCloverField *clover, double kappa, const GaugeField *gaugeSloppy, const MugiqHipCloverField *cloverSloppy,
                         const std::vector<MugiqHipTransfer> &transfersSloppy, const std::vector<MugiqHipCoarseOperator> &coarseOpsSloppy,
                         const std::vector<MgSolveParam> &params, std::vector<int> &iters, std::vector<double> &relres,
                         std::vector<std::vector<double>> *history = nullptr, int *hostReads = nullptr, const MugiqHipComm *comm = nullptr,
                         void *stream = nullptr) {
  if (b.empty() || x.size() != b.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgSolveMixed: size mismatch");
  const int L = detail::mgLevels(transfersSloppy, coarseOpsSloppy, params, "mgSolveMixed");
  int stride;
  std::vector<double> hist = detail::mgOutputs(b.size(), params[0].maxIter, history != nullptr, iters, relres, &stride);
  const int st = mugiq_hip_mg_solve_mixed_levels(x.data(), b.data(), (int)b.size(), &gauge, clover, kappa, gaugeSloppy, cloverSloppy, transfersSloppy.data(),
                                                 coarseOpsSloppy.data(), L, params.data(), iters.data(), relres.data(), history ? hist.data() : nullptr,
                                                 stride, hostReads, comm, stream);
  return detail::mgHistory(st, hist, stride, iters, history);
}
// dst_i = src_i between spinor fields of either precision (mugiq_hip_mg_convert_precision)
inline void mgConvertPrecision(const std::vector<ColorSpinorField> &dst, const std::vector<ColorSpinorField> &src, void *stream = nullptr) {
  if (src.empty() || dst.size() != src.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgConvertPrecision: size mismatch");
  check(mugiq_hip_mg_convert_precision(dst.data(), src.data(), (int)src.size(), stream));
}
// dst.V = src.V between two transfers of equal geometry and either precision (mugiq_hip_transfer_convert): the sloppy hierarchy's V
inline void transferConvert(const MugiqHipTransfer &dst, const MugiqHipTransfer &src, void *stream = nullptr) {
  check(mugiq_hip_transfer_convert(&dst, &src, stream));
}
// ---- the MG setup (csrc/mg_setup.hip; new) ----
// Orthonormalise the columns of V inside every (aggregate, coarse spin) block, in place (mugiq_hip_block_orthonormalize).  Returns the
// info; a minPivotRatio below rankTol throws (status 1) with V filled all the same
inline MugiqHipBlockOrthoInfo blockOrthonormalize(const MugiqHipTransfer &transfer, int nPasses = 2, double rankTol = 0.0, void *stream = nullptr) {
  MugiqHipBlockOrthoInfo info{};
  check(mugiq_hip_block_orthonormalize(&transfer, nPasses, rankTol, &info, stream));
  return info;
}
// max over the blocks of max |B^dag B - 1| (mugiq_hip_transfer_orthonormality)
inline double transferOrthonormality(const MugiqHipTransfer &transfer, void *stream = nullptr) {
  double out = 0.0;
  check(mugiq_hip_transfer_orthonormality(&transfer, &out, stream));
  return out;
}
// MugiqHipMgSetupParam with the defaults of mugiq_hip_mg_setup_param_default (setupMaxIter and setupTol as in tests/loop.cpp, the rest
// first guesses)
struct MgSetupParam : MugiqHipMgSetupParam {
  MgSetupParam() { check(mugiq_hip_mg_setup_param_default(this)); }
};
// V of `transfer` (written in place) and, if coarseOp is given, its coarse operator from the gauge field and the caller's start vectors
// (mugiq_hip_mg_setup)
inline MugiqHipMgSetupInfo mgSetup(const MugiqHipTransfer &transfer, CoarseOperator *coarseOp, const std::vector<ColorSpinorField> &start,
                                   const GaugeField &gauge, const MugiqHipCloverField *clover, double kappa, const MgSetupParam &param = MgSetupParam(),
                                   const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (start.empty()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgSetup: no start vectors");
  MugiqHipMgSetupInfo info{};
  check(mugiq_hip_mg_setup(&transfer, coarseOp ? coarseOp->desc() : nullptr, start.data(), (int)start.size(), &gauge, clover, kappa, &param, &info, comm,
                           stream));
  return info;
}
// ---- the coarse-grid eigensolver (csrc/coarse_eig.hip, csrc/dense_herm.cpp; new) ----
// G[i * b.size() + j] = <a_i, b_j> on the matrix pipe, fixed-order sums, one blocking read (mugiq_hip_coarse_gram)
inline std::vector<std::complex<double>> coarseGram(const std::vector<MugiqHipCoarseField> &a, const std::vector<MugiqHipCoarseField> &b,
                                                    const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (a.empty() || b.empty()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "coarseGram: no vectors");
  std::vector<std::complex<double>> G(a.size() * b.size());
  check(mugiq_hip_coarse_gram(reinterpret_cast<double *>(G.data()), a.data(), (int)a.size(), b.data(), (int)b.size(), comm, stream));
  return G;
}
// out_j = sum_i in_i Z[i * out.size() + j], out of place (mugiq_hip_coarse_rotate)
inline void coarseRotate(const std::vector<MugiqHipCoarseField> &out, const std::vector<MugiqHipCoarseField> &in, const std::vector<std::complex<double>> &Z,
                         const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (in.empty() || out.empty() || Z.size() != in.size() * out.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "coarseRotate: size mismatch");
  check(mugiq_hip_coarse_rotate(out.data(), (int)out.size(), in.data(), (int)in.size(), reinterpret_cast<const double *>(Z.data()), comm, stream));
}
// (H + H^dag) / 2 = Z diag(theta) Z^dag on the host, theta ascending; H and Z row-major n x n (mugiq_hip_hermitian_eigh)
inline void hermitianEigh(int n, const std::vector<std::complex<double>> &H, std::vector<double> &theta, std::vector<std::complex<double>> &Z) {
  if (n < 1 || H.size() < (size_t)n * n) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "hermitianEigh: size mismatch");
  theta.assign(n, 0.0);
  Z.assign((size_t)n * n, std::complex<double>(0.0, 0.0));
  check(mugiq_hip_hermitian_eigh(n, reinterpret_cast<const double *>(H.data()), theta.data(), reinterpret_cast<double *>(Z.data())));
}
// R with G = R^dag R, and R^-1 (mugiq_hip_cholesky_upper, mugiq_hip_upper_triangular_inverse); a pivot <= rankTol max diag G throws (status 1)
inline void choleskyUpper(int n, const std::vector<std::complex<double>> &G, std::vector<std::complex<double>> &R, double rankTol = 0.0) {
  if (n < 1 || G.size() < (size_t)n * n) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "choleskyUpper: size mismatch");
  R.assign((size_t)n * n, std::complex<double>(0.0, 0.0));
  check(mugiq_hip_cholesky_upper(n, reinterpret_cast<const double *>(G.data()), reinterpret_cast<double *>(R.data()), rankTol, nullptr, nullptr));
}
inline void upperTriangularInverse(int n, const std::vector<std::complex<double>> &R, std::vector<std::complex<double>> &Rinv) {
  if (n < 1 || R.size() < (size_t)n * n) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "upperTriangularInverse: size mismatch");
  Rinv.assign((size_t)n * n, std::complex<double>(0.0, 0.0));
  check(mugiq_hip_upper_triangular_inverse(n, reinterpret_cast<const double *>(R.data()), reinterpret_cast<double *>(Rinv.data())));
}
// MugiqHipCoarseEigParam with the defaults of mugiq_hip_coarse_eig_param_default (the members the reference's tests/eigensolve.cpp
// fills from QUDA's flags; the values are first guesses, not tuned)
struct CoarseEigParam : MugiqHipCoarseEigParam {
  CoarseEigParam() { check(mugiq_hip_coarse_eig_param_default(this)); }
};
// The param.nConv lowest eigenpairs of A = MdagM | MMdag of the explicit coarse operator into eVecs (param.nConv fields), from the
// caller's param.nKr start vectors (mugiq_hip_coarse_eigensolve).  maxIter exhausted throws (status 5) unless allowUnconverged: the
// outputs are filled all the same, and info.nConverged says how far it got
inline MugiqHipCoarseEigInfo coarseEigensolve(const std::vector<MugiqHipCoarseField> &eVecs, const std::vector<MugiqHipCoarseField> &start,
                                              const CoarseOperator &op, int opType, const CoarseEigParam &param, std::vector<double> &theta,
                                              std::vector<double> &residual, std::vector<double> &sigma, bool allowUnconverged = false,
                                              const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if ((int)eVecs.size() != param.nConv || (int)start.size() != param.nKr || eVecs.empty())
    throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "coarseEigensolve: nConv eigenvector fields and nKr start vectors are needed");
  theta.assign(eVecs.size(), 0.0);
  residual.assign(eVecs.size(), 0.0);
  sigma.assign(eVecs.size(), 0.0);
  MugiqHipCoarseEigInfo info{};
  const int st = mugiq_hip_coarse_eigensolve(eVecs.data(), start.data(), op.desc(), opType, &param, theta.data(), residual.data(), sigma.data(), &info,
                                             comm, stream);
  if (!(st == MUGIQ_HIP_ERROR_NOT_CONVERGED && allowUnconverged)) check(st);
  return info;
}
// ---- ... on a process grid (mugiq_hip_coarse_gram_grid, mugiq_hip_coarse_eigensolve_grid; new): the same two names with the operator's
// MugiqHipCoarseHalo behind the vectors / the operator and a comm that is required.  The Gram matrix needs nothing of the halo; it marks
// the vectors as the local blocks of the grid the halo was built on.  coarseRotate has no grid form: a rotation is local to a rank
inline std::vector<std::complex<double>> coarseGram(const std::vector<MugiqHipCoarseField> &a, const std::vector<MugiqHipCoarseField> &b,
                                                    const MugiqHipCoarseHalo &, const MugiqHipComm *comm, void *stream = nullptr) {
  if (a.empty() || b.empty()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "coarseGram: no vectors");
  std::vector<std::complex<double>> G(a.size() * b.size());
  check(mugiq_hip_coarse_gram_grid(reinterpret_cast<double *>(G.data()), a.data(), (int)a.size(), b.data(), (int)b.size(), comm, stream));
  return G;
}
inline MugiqHipCoarseEigInfo coarseEigensolve(const std::vector<MugiqHipCoarseField> &eVecs, const std::vector<MugiqHipCoarseField> &start,
                                              const CoarseOperator &op, const MugiqHipCoarseHalo &halo, int opType, const CoarseEigParam &param,
                                              std::vector<double> &theta, std::vector<double> &residual, std::vector<double> &sigma,
                                              MugiqHipCoarseEigGridInfo &gridInfo, const MugiqHipComm *comm, bool allowUnconverged = false,
                                              void *stream = nullptr) {
  if ((int)eVecs.size() != param.nConv || (int)start.size() != param.nKr || eVecs.empty())
    throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "coarseEigensolve: nConv eigenvector fields and nKr start vectors are needed");
  theta.assign(eVecs.size(), 0.0);
  residual.assign(eVecs.size(), 0.0);
  sigma.assign(eVecs.size(), 0.0);
  MugiqHipCoarseEigInfo info{};
  const int st = mugiq_hip_coarse_eigensolve_grid(eVecs.data(), start.data(), op.desc(), &halo, opType, &param, theta.data(), residual.data(),
                                                  sigma.data(), &info, &gridInfo, comm, stream);
  if (!(st == MUGIQ_HIP_ERROR_NOT_CONVERGED && allowUnconverged)) check(st);
  return info;
}
// x_r = M^-1 b_r by CG on the normal equations from the low-mode start (mugiq_hip_wilson_solve).  Returns false where a right-hand
// side did not reach tol within maxIter (x, iters and relres are filled all the same); every other failure throws.
inline bool wilsonSolve(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, const GaugeField &gauge, double kappa,
                        const std::vector<ColorSpinorField> &eVecs, const std::vector<double> &sigma, double tol, int maxIter,
                        std::vector<int> &iters, std::vector<double> &relres, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (b.empty() || x.size() != b.size() || sigma.size() != eVecs.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "wilsonSolve: size mismatch");
  iters.assign(b.size(), 0);
  relres.assign(b.size(), 0.0);
  const int st = mugiq_hip_wilson_solve(x.data(), b.data(), (int)b.size(), &gauge, kappa, eVecs.empty() ? nullptr : eVecs.data(),
                                        eVecs.empty() ? nullptr : sigma.data(), (int)eVecs.size(), tol, maxIter, iters.data(), relres.data(), comm,
                                        stream);
  if (st == MUGIQ_HIP_ERROR_NOT_CONVERGED) return false;
  check(st);
  return true;
}
// ---- stout smearing, border refresh and plaquette of the border-extended gauge field (csrc/smear.hip; new) ----
// the R-deep borders of a device-resident field from its interior (exchangeExtendedGhost, lib/displace.cpp:127)
inline void exchangeExtendedGauge(const GaugeField &gauge, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  check(mugiq_hip_exchange_extended_gauge(&gauge, comm, stream));
}
// nSteps stout steps of `in` into `out` (same geometry and precision, no overlap); smearDims 3: spatial links and staples only, 4: all
inline void stoutSmear(const GaugeField &out, const GaugeField &in, double rho, int nSteps, int smearDims = 3, const MugiqHipComm *comm = nullptr,
                       void *stream = nullptr) {
  check(mugiq_hip_stout_smear(&out, &in, rho, nSteps, smearDims, comm, stream));
}
// {mean, spatial, temporal} of Re tr P / 3 over all ranks, what the reference prints after plaqQuda (tests/loop.cpp:895-898)
inline std::array<double, 3> plaquette(const GaugeField &gauge, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  std::array<double, 3> plaq{};
  check(mugiq_hip_plaquette(&gauge, plaq.data(), comm, stream));
  return plaq;
}
// ---- the clover term (csrc/clover.hip; new): a device field the holder owns, and the three calls above for the Wilson-clover operator ----
class CloverField {
public:
  CloverField(const int X[4], int precision) { check(mugiq_hip_alloc_clover(&f_, X, precision)); }
  ~CloverField() { mugiq_hip_free_clover(&f_); }
  CloverField(const CloverField &) = delete;
  CloverField &operator=(const CloverField &) = delete;
  // A(x) from the border-extended links; coeff = kappa * c_sw (QUDA's clover_coeff).  The gauge precision of the operator calls must be
  // this field's.
  void compute(const GaugeField &gauge, double coeff, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
    check(mugiq_hip_compute_clover(&f_, &gauge, coeff, comm, stream));
  }
  const MugiqHipCloverField *desc() const { return &f_; }
  static size_t bytes(const int X[4], int precision) { return mugiq_hip_clover_bytes(X, precision); }

private:
  MugiqHipCloverField f_{};
};
inline void wilsonApply(const std::vector<ColorSpinorField> &dst, const std::vector<ColorSpinorField> &src, const GaugeField &gauge,
                        const CloverField &clover, double kappa, int opType = MUGIQ_HIP_EIG_OPERATOR_M, double scale = 1.0,
                        const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (src.empty() || dst.size() != src.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "wilsonApply: size mismatch");
  check(mugiq_hip_wilson_clover_apply(dst.data(), src.data(), (int)src.size(), &gauge, clover.desc(), kappa, opType, scale, comm, stream));
}
namespace detail {
// clover NULL: the unimproved operator
inline void computeEvals(const std::vector<ColorSpinorField> &eVecs, const GaugeField &gauge, const MugiqHipCloverField *clover, double kappa,
                         int opType, bool massNormalization, std::vector<std::complex<double>> &lambda, std::vector<double> &residual,
                         std::vector<double> &sigma, const MugiqHipComm *comm, void *stream) {
  if (eVecs.empty()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "computeEvals: no eigenvectors");
  lambda.assign(eVecs.size(), std::complex<double>(0.0, 0.0));
  residual.assign(eVecs.size(), 0.0);
  sigma.assign(eVecs.size(), 0.0);
  check(mugiq_hip_compute_evals_clover(eVecs.data(), (int)eVecs.size(), &gauge, clover, kappa, opType, massNormalization ? 1 : 0,
                                       reinterpret_cast<double *>(lambda.data()), residual.data(), sigma.data(), comm, stream));
  if (opType == MUGIQ_HIP_EIG_OPERATOR_M || opType == MUGIQ_HIP_EIG_OPERATOR_MDAG) sigma.clear();
}
inline bool wilsonSolve(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, const GaugeField &gauge,
                        const MugiqHipCloverField *clover, double kappa, const std::vector<ColorSpinorField> &eVecs, const std::vector<double> &sigma,
                        double tol, int maxIter, std::vector<int> &iters, std::vector<double> &relres, const MugiqHipComm *comm, void *stream) {
  if (b.empty() || x.size() != b.size() || sigma.size() != eVecs.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "wilsonSolve: size mismatch");
  iters.assign(b.size(), 0);
  relres.assign(b.size(), 0.0);
  const int st = mugiq_hip_wilson_clover_solve(x.data(), b.data(), (int)b.size(), &gauge, clover, kappa, eVecs.empty() ? nullptr : eVecs.data(),
                                               eVecs.empty() ? nullptr : sigma.data(), (int)eVecs.size(), tol, maxIter, iters.data(),
                                               relres.data(), comm, stream);
  if (st == MUGIQ_HIP_ERROR_NOT_CONVERGED) return false;
  check(st);
  return true;
}
}  // namespace detail
inline void computeEvals(const std::vector<ColorSpinorField> &eVecs, const GaugeField &gauge, const CloverField &clover, double kappa, int opType,
                         bool massNormalization, std::vector<std::complex<double>> &lambda, std::vector<double> &residual,
                         std::vector<double> &sigma, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  detail::computeEvals(eVecs, gauge, clover.desc(), kappa, opType, massNormalization, lambda, residual, sigma, comm, stream);
}
// (v_n, sigma_n): eigenpairs of H = g5 M_clov
inline bool wilsonSolve(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, const GaugeField &gauge,
                        const CloverField &clover, double kappa, const std::vector<ColorSpinorField> &eVecs, const std::vector<double> &sigma,
                        double tol, int maxIter, std::vector<int> &iters, std::vector<double> &relres, const MugiqHipComm *comm = nullptr,
                        void *stream = nullptr) {
  return detail::wilsonSolve(x, b, gauge, clover.desc(), kappa, eVecs, sigma, tol, maxIter, iters, relres, comm, stream);
}
// The members of the reference's Eigsolve_Mugiq (include/eigsolve_mugiq.h) that work on eigenvectors somebody else computed
class Eigsolve_Mugiq {
public:
  // the Wilson-clover operator: `clover` must outlive the object
  Eigsolve_Mugiq(std::vector<ColorSpinorField> eVecs, const GaugeField &gauge, const CloverField &clover, double kappa, int opType,
                 const MugiqHipComm *comm = nullptr, bool massNormalization = false, void *stream = nullptr)
      : Eigsolve_Mugiq(std::move(eVecs), gauge, kappa, opType, comm, massNormalization, stream) {
    clover_ = clover.desc();
  }
  Eigsolve_Mugiq(std::vector<ColorSpinorField> eVecs, const GaugeField &gauge, double kappa, int opType, const MugiqHipComm *comm = nullptr,
                 bool massNormalization = false, void *stream = nullptr)
      : eVecs_(std::move(eVecs)), gauge_(gauge), kappa_(kappa), opType_(opType), comm_(comm), mass_(massNormalization), stream_(stream),
        eVals_quda_(eVecs_.size()) {}
  // the computeCoarse branch (lib/eigsolve_mugiq.cpp:27-33) on the explicit coarse operator: coarse eigenvectors (may be empty until
  // computeEvecs has run), the finest-level transfer and the operator built from it for this gauge field, clover field (NULL: Wilson) and
  // kappa.  `coarseOp` must outlive the object.  computeEvals, computeEvecs and printEvals work; projectVector and solve are fine-level
  Eigsolve_Mugiq(std::vector<MugiqHipCoarseField> coarseEvecs, const MugiqHipTransfer &transfer, const CoarseOperator &coarseOp, const GaugeField &gauge,
                 const MugiqHipCloverField *clover, double kappa, int opType = MUGIQ_HIP_EIG_OPERATOR_MDAGM, const MugiqHipComm *comm = nullptr,
                 bool massNormalization = false, void *stream = nullptr)
      : gauge_(gauge), clover_(clover), kappa_(kappa), opType_(opType), comm_(comm), mass_(massNormalization), stream_(stream),
        eVals_quda_(coarseEvecs.size()), coarseEvecs_(std::move(coarseEvecs)), coarseOp_(&coarseOp) {
    (void)transfer;  // named for the reader: the operator was built from it and carries everything the calls below need
  }
  void computeEvals() {
    if (coarseOp_) {
      mugiq_hip::computeEvalsCoarse(coarseEvecs_, *coarseOp_, opType_, mass_, eVals_, evals_res_, eVals_sigma_, comm_, stream_);
      return;
    }
    detail::computeEvals(eVecs_, gauge_, clover_, kappa_, opType_, mass_, eVals_, evals_res_, eVals_sigma_, comm_, stream_);
  }
  // Eigsolve_Mugiq::computeEvecs (lib/eigsolve_mugiq.cpp:278-287) for the coarse-operator constructor: the param.nConv lowest eigenpairs of
  // this object's operator (MdagM | MMdag) by coarseEigensolve, into the caller's fields eVecs, which become the object's eigenvectors;
  // eVals_quda takes the solver's theta, so that printEvals shows it beside what computeEvals recomputes
  MugiqHipCoarseEigInfo computeEvecs(const std::vector<MugiqHipCoarseField> &eVecs, const std::vector<MugiqHipCoarseField> &start,
                                     const CoarseEigParam &param = CoarseEigParam(), bool allowUnconverged = false) {
    if (!coarseOp_) throw Error(MUGIQ_HIP_ERROR_UNSUPPORTED, "Eigsolve_Mugiq::computeEvecs: needs the coarse-operator constructor (fine-operator eigensolves are out of scope)");
    std::vector<double> theta, res, sig;
    const MugiqHipCoarseEigInfo info = coarseEigensolve(eVecs, start, *coarseOp_, opType_, param, theta, res, sig, allowUnconverged, comm_, stream_);
    coarseEvecs_ = eVecs;
    eVals_quda_.assign(theta.begin(), theta.end());
    eVals_.assign(theta.size(), std::complex<double>(0.0, 0.0));
    evals_res_.assign(theta.size(), 0.0);
    eVals_sigma_.clear();
    return info;
  }
  std::vector<MugiqHipCoarseField> &getCoarseEvecs() { return coarseEvecs_; }
  // lib/eigsolve_mugiq.cpp:317-337, the two line formats character for character (the interface contract of its log)
  void printEvals(FILE *out = stdout) const {
    if (comm_ && comm_->rank != 0) return;
    fprintf(out, "\nEigsolve_Mugiq - Eigenvalues:\n");
    for (size_t i = 0; i < eVals_.size(); i++)
      fprintf(out, "Mugiq-Quda: Eval[%04d] = %+.16e %+.16e , %+.16e %+.16e , Residual = %+.16e\n", (int)i, eVals_[i].real(), eVals_[i].imag(),
              eVals_quda_[i].real(), eVals_quda_[i].imag(), evals_res_[i]);
    if (opType_ == MUGIQ_HIP_EIG_OPERATOR_MDAGM || opType_ == MUGIQ_HIP_EIG_OPERATOR_MMDAG) {
      fprintf(out, "\n");
      for (size_t i = 0; i < eVals_sigma_.size(); i++) fprintf(out, "Mugiq-Quda: Sigma[%04d] = %+.16e\n", (int)i, eVals_sigma_[i]);
    }
  }
  void projectVector(ColorSpinorField &out, ColorSpinorField &in) { mugiq_hip::projectVector(out, in, eVecs_, comm_, stream_); }
  // M^-1 b; with opType H the eigenpairs (sigma of computeEvals) deflate the start vector
  bool solve(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, double tol, int maxIter, std::vector<int> &iters,
             std::vector<double> &relres) {
    const bool defl = opType_ == MUGIQ_HIP_EIG_OPERATOR_H && eVals_sigma_.size() == eVecs_.size();
    static const std::vector<ColorSpinorField> none;
    static const std::vector<double> noSigma;
    return detail::wilsonSolve(x, b, gauge_, clover_, kappa_, defl ? eVecs_ : none, defl ? eVals_sigma_ : noSigma, tol, maxIter, iters, relres, comm_,
                               stream_);
  }
  std::vector<ColorSpinorField> &getEvecs() { return eVecs_; }
  std::vector<std::complex<double>> *getEvals() { return &eVals_; }
  std::vector<std::complex<double>> *getEvalsQuda() { return &eVals_quda_; }
  std::vector<double> *getEvalsRes() { return &evals_res_; }
  std::vector<double> *getEvalsSigma() { return &eVals_sigma_; }

private:
  std::vector<ColorSpinorField> eVecs_;
  GaugeField gauge_;
  const MugiqHipCloverField *clover_ = nullptr;  // NULL: the unimproved operator
  double kappa_;
  int opType_;
  const MugiqHipComm *comm_;
  bool mass_;
  void *stream_;
  std::vector<std::complex<double>> eVals_, eVals_quda_;
  std::vector<double> evals_res_, eVals_sigma_;
  std::vector<MugiqHipCoarseField> coarseEvecs_;  // the computeCoarse branch
  const CoarseOperator *coarseOp_ = nullptr;
};

// lib/contract_wrappers.cu:133-156
template <typename Float>
inline void convertIdxOrder_mapGamma(std::complex<Float> *dataPosMP_d, const std::complex<Float> *dataPos_d, int nData, int nLoop,
                                     int nParity, int volumeCB, const int localL[], void *stream = nullptr) {
  check(mugiq_hip_convert_idx_order_map_gamma(dataPosMP_d, dataPos_d, nData, nLoop, nParity, volumeCB, localL, precisionOf<Float>(),
                                              stream));
}

// lib/contract_wrappers.cu:171-198 (the halo exchange of :166-169 is the caller's: fill src->ghost first)
template <typename Float, int order>
inline void performCovariantDisplacementVector(ColorSpinorField *dst, ColorSpinorField *src, GaugeField *gauge, DisplaceDir dispDir,
                                               DisplaceSign dispSign, const int commDim[4] = nullptr, void *stream = nullptr) {
  checkField<Float, order>(dst, "performCovariantDisplacementVector");
  checkField<Float, order>(src, "performCovariantDisplacementVector");
  check(mugiq_hip_perform_covariant_displacement_vector(dst, src, gauge, (int)dispDir, (int)dispSign, commDim, stream));
}

// the cublas{Z,C}gemm of lib/loop_mugiq.cpp:363-378
template <typename Float>
inline void momentumProjectionGemm(std::complex<Float> *dataMom_d, const std::complex<Float> *dataPosMP_d,
                                   const std::complex<Float> *phaseMatrix_d, int locT, int nData, long long locV3, int Nmom,
                                   void *stream = nullptr) {
  check(mugiq_hip_momentum_projection(dataMom_d, dataPosMP_d, phaseMatrix_d, locT, nData, locV3, Nmom, precisionOf<Float>(), nullptr,
                                      0, stream));
}

// include/gamma.h:11-20
inline std::string GammaName(int m) {
  const char *s = mugiq_hip_gamma_name(m);
  if (!s) throw std::out_of_range("GammaName");
  return s;
}

// The members of QudaGaugeParam this path reads (lib/displace.cpp:70-99: local lattice, host and device precision).
// Inside a QUDA build (MUGIQ_HIP_WITH_QUDA, see mugiq_hip_quda_adapter.hpp) it IS QudaGaugeParam: same member names.
#ifdef MUGIQ_HIP_WITH_QUDA
using GaugeParam = QudaGaugeParam;
#else
struct GaugeParam {
  int X[4];       // local lattice dimensions
  int cpu_prec;   // precision of the host links: 4 | 8 (QUDA_SINGLE/DOUBLE_PRECISION have these values)
  int cuda_prec;  // precision of the device field: must equal sizeof(Float) of the loop (lib/displace.cpp:84-87)
};
#endif

// include/mugiq.h:28-47, member for member: `gauge` are the four host arrays of the LOCAL lattice in QDP order
// (gauge[dir][(parity*V/2 + x_cb)*18 + (row*3+col)*2 + re/im], tests/loop.cpp:88,106,902-918) and `gauge_param` their
// description; Loop_Mugiq builds the border-extended device field from them as Displace does (lib/displace.cpp:70-134).
// gauge_ext (not in the reference) hands over an extended device field that already exists instead.
struct MugiqLoopParam {
  int Nmom = 0;
  std::vector<std::vector<int>> momMatrix;  // [Nmom][3]
  LoopFTSign FTSign = LOOP_FT_SIGN_PLUS;
  LoopCalcType calcType = LOOP_CALC_TYPE_OPT_KERNEL;
  MuGiqBool writeMomSpaceHDF5 = MUGIQ_BOOL_FALSE;
  MuGiqBool writePosSpaceHDF5 = MUGIQ_BOOL_FALSE;
  MuGiqBool doMomProj = MUGIQ_BOOL_FALSE;
  MuGiqBool doNonLocal = MUGIQ_BOOL_FALSE;
  std::vector<std::string> disp_entry;
  std::vector<std::string> disp_str;
  std::string fname_mom_h5;
  std::string fname_pos_h5;
  std::vector<int> disp_start;
  std::vector<int> disp_stop;
  void *gauge[4] = {nullptr, nullptr, nullptr, nullptr};
  GaugeParam *gauge_param = nullptr;
  const GaugeField *gauge_ext = nullptr;
  int loopPrecision = 0;  // not in the reference: 8 over fp32 eigenvectors = mixed precision
};

// tests/loop.cpp:656-705
inline void setDisplaceEntryString(MugiqLoopParam &p, const std::string &entries) {
  const int maxE = 64;
  std::vector<char> strs(4 * maxE);
  std::vector<int> a(maxE), b(maxE);
  int n = mugiq_hip_parse_displace_entry_string(entries.c_str(), maxE, strs.data(), a.data(), b.data());
  if (n < 0) check(-n);
  p.disp_entry.clear();
  p.disp_str.clear();
  p.disp_start.assign(a.begin(), a.begin() + n);
  p.disp_stop.assign(b.begin(), b.begin() + n);
  size_t pos = 0;
  for (int i = 0; i < n; i++) {
    p.disp_str.emplace_back(&strs[4 * i]);
    size_t semi = entries.find(';', pos);
    p.disp_entry.push_back(entries.substr(pos, semi == std::string::npos ? std::string::npos : semi - pos));
    pos = semi == std::string::npos ? entries.size() : semi + 1;
  }
  p.doNonLocal = MUGIQ_BOOL_TRUE;
}

// lib/contract_wrappers.cu:166-169: depth-1 ghost zones of every partitioned dimension, both directions
inline void exchangeGhostVec(ColorSpinorField *x, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  check(mugiq_hip_exchange_ghost_vec(x, comm, stream));
}

// include/displace.h:13-80, lib/displace.cpp: the displacement state machine Loop_Mugiq drives (its friend in the reference;
// public here so that the reference's loop nest, lib/loop_mugiq.cpp:455-509, can be written against it call for call).
// `comm` stands for QUDA's communicator (commDimPartitioned), NULL = one process.
template <typename Float, int fieldOrder> class Displace {
  const std::vector<std::string> DisplaceFlagArray{"+x", "-x", "+y", "-y", "+z", "-z", "+t", "-t"};  // include/displace.h:21
  const char *DisplaceDirArray[4] = {"x", "y", "z", "t"};
  const char *DisplaceSignArray[2] = {"-", "+"};
  std::string dispString;
  DisplaceFlag dispFlag = DispFlagNone;
  DisplaceDir dispDir = DispDirNone;
  DisplaceSign dispSign = DispSignNone;
  GaugeField ownGauge_{};            // gaugeField when built here from loopParams.gauge[4]
  const GaugeField *gaugeField = nullptr;
  ColorSpinorField auxDispVec{};
  const MugiqHipComm *comm_;
  void *stream_;
  int commDim_[4], exRng[4];

public:
  Displace(MugiqLoopParam *lp, const ColorSpinorField *csf, int coarsePrec = 0, const MugiqHipComm *comm = nullptr, void *stream = nullptr)
      : comm_(comm), stream_(stream) {
    checkField<Float, fieldOrder>(csf, "Displace");
    for (int d = 0; d < 4; d++) {
      commDim_[d] = (comm && (comm->grid[d] > 1 || comm->partitioned[d])) ? 1 : 0;  // comm_dim_partitioned(d), forced included
      exRng[d] = 2 * commDim_[d];  // lib/displace.cpp:16
    }
    if (lp->gauge_ext) gaugeField = lp->gauge_ext;
    else {
      if (!lp->gauge[0] || !lp->gauge_param) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "Displace: loopParams holds no gauge field");
      const GaugeParam &gp = *lp->gauge_param;
      if ((int)gp.cuda_prec != precisionOf<Float>())
        throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "createCudaGaugeField: Incompatible precision settings between Displace template and gauge field parameters");
      int X[4];
      for (int d = 0; d < 4; d++) X[d] = gp.X[d];
      check(mugiq_hip_alloc_extended_gauge(&ownGauge_, X, exRng, precisionOf<Float>()));
      const void *links[4] = {lp->gauge[0], lp->gauge[1], lp->gauge[2], lp->gauge[3]};
      const int st = mugiq_hip_create_extended_gauge(&ownGauge_, links, (int)gp.cpu_prec, comm, stream);
      if (st) {
        mugiq_hip_free_extended_gauge(&ownGauge_);
        check(st);
      }
      gaugeField = &ownGauge_;
    }
    check(mugiq_hip_alloc_spinor_like(&auxDispVec, csf, coarsePrec, nullptr));  // QUDA_ZERO_FIELD_CREATE, lib/displace.cpp:26-30
  }
  ~Displace() {
    mugiq_hip_free_spinor(&auxDispVec);
    if (ownGauge_.data) mugiq_hip_free_extended_gauge(&ownGauge_);
  }
  Displace(const Displace &) = delete;
  Displace &operator=(const Displace &) = delete;

  // lib/displace.cpp:137-152
  DisplaceFlag WhichDisplaceFlag() const {
    for (int i = 0; i < (int)DisplaceFlagArray.size(); i++)
      if (dispString == DisplaceFlagArray[i]) return static_cast<DisplaceFlag>(i);
    throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "WhichDisplaceFlag: Cannot parse given displacement string = " + dispString + ".");
  }
  DisplaceDir WhichDisplaceDir() const { return static_cast<DisplaceDir>((int)dispFlag / 2); }                          // :155-180
  DisplaceSign WhichDisplaceSign() const { return ((int)dispFlag % 2 == 0) ? DispSignPlus : DispSignMinus; }           // :182-203
  // lib/displace.cpp:206-223
  void setupDisplacement(const std::string &dStr) {
    dispString = dStr;
    dispFlag = WhichDisplaceFlag();
    dispDir = WhichDisplaceDir();
    dispSign = WhichDisplaceSign();
    int d = -1, sg = -1;
    check(mugiq_hip_parse_displacement(dStr.c_str(), &d, &sg));  // the library's table must agree
    if (d != (int)dispDir || sg != (int)dispSign) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "setupDisplacement: Got invalid dispDir and/or dispSign.");
  }
  DisplaceDir dir() const { return dispDir; }
  DisplaceSign sign() const { return dispSign; }
  const GaugeField *gauge() const { return gaugeField; }
  // lib/displace.cpp:40-52
  void resetAuxDispVec(const ColorSpinorField *fineEvec) { check(mugiq_hip_copy_spinor(&auxDispVec, fineEvec, stream_)); }
  void swapAuxDispVec(ColorSpinorField *displacedEvec) { check(mugiq_hip_copy_spinor(displacedEvec, &auxDispVec, stream_)); }
  // lib/displace.cpp:55-67 (+ the exchangeGhostVec of lib/contract_wrappers.cu:178): displacedEvec <- D_{dir,sign} displacedEvec
  void doVectorDisplacement(DisplaceType dispType, ColorSpinorField *displacedEvec, int /*idisp*/) {
    if (dispType != DISPLACE_TYPE_COVARIANT) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "Unsupported Displacement type " + std::to_string((int)dispType));
    if (dispDir == DispDirNone) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "doVectorDisplacement: Got invalid dispDir and/or dispSign.");
    check(mugiq_hip_zero_spinor(&auxDispVec, stream_));
    exchangeGhostVec(displacedEvec, comm_, stream_);
    ColorSpinorField aux = auxDispVec;
    performCovariantDisplacementVector<Float, fieldOrder>(&aux, displacedEvec, const_cast<GaugeField *>(gaugeField), dispDir, dispSign, commDim_, stream_);
    swapAuxDispVec(displacedEvec);
  }
};

// include/loop_mugiq.h:123-134: Loop_Mugiq(loopParams, eigsolve); computeCoarseLoop(); writeLoopsHDF5()
// `eVecs` / `eVals_sigma` are what the reference reads from Eigsolve_Mugiq as a friend (lib/loop_mugiq.cpp:442,479).
template <typename Float, int fieldOrder> class Loop_Mugiq {
  MugiqHipLoop *h_ = nullptr;
  int nEv_ = 0;  // eigenvectors of a one-sided loop, fine-level or coarse (what deflate / deflateCoarse read); 0 for two-sided loops
  GaugeField ownGauge_{};  // Displace::gaugeField when built here from loopParams.gauge[4]

  // everything the C parameter block points into, alive for the duration of the create call
  struct CParam {
    std::vector<int> mom;
    std::vector<const char *> ent, str;
    MugiqHipLoopParam p{};
  };
  void fill(CParam &c, MugiqLoopParam *lp, const MugiqHipComm *comm, void *stream) {
    for (auto &m : lp->momMatrix) {
      if (m.size() != 3) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "Loop_Mugiq: momMatrix rows must have 3 entries");
      c.mom.insert(c.mom.end(), m.begin(), m.end());
    }
    for (auto &s : lp->disp_entry) c.ent.push_back(s.c_str());
    for (auto &s : lp->disp_str) c.str.push_back(s.c_str());
    c.ent.resize(c.str.size(), "");
    if (lp->disp_str.size() != lp->disp_start.size() || lp->disp_str.size() != lp->disp_stop.size())
      throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "Displacement string length not compatible with displacement limits length");
    MugiqHipLoopParam &p = c.p;
    p.Nmom = lp->Nmom ? lp->Nmom : (int)lp->momMatrix.size();
    p.momMatrix = c.mom.empty() ? nullptr : c.mom.data();
    p.FTSign = (int)lp->FTSign;
    p.calcType = (int)lp->calcType;
    p.writeMomSpaceHDF5 = lp->writeMomSpaceHDF5 == MUGIQ_BOOL_TRUE;
    p.writePosSpaceHDF5 = lp->writePosSpaceHDF5 == MUGIQ_BOOL_TRUE;
    p.doMomProj = lp->doMomProj == MUGIQ_BOOL_TRUE;
    p.doNonLocal = lp->doNonLocal == MUGIQ_BOOL_TRUE;
    p.nDispEntries = (int)c.str.size();
    p.disp_entry = c.ent.data();
    p.disp_str = c.str.data();
    p.disp_start = lp->disp_start.data();
    p.disp_stop = lp->disp_stop.data();
    p.fname_mom_h5 = lp->fname_mom_h5.c_str();
    p.fname_pos_h5 = lp->fname_pos_h5.c_str();
    p.loopPrecision = lp->loopPrecision;
    p.gauge = lp->gauge_ext;
    if (p.doNonLocal && p.nDispEntries > 0 && !p.gauge && lp->gauge[0] && lp->gauge_param) {
      // Displace::Displace + createExtendedCudaGaugeField (lib/displace.cpp:6-37,70-134)
      const GaugeParam &gp = *lp->gauge_param;
      if ((int)gp.cuda_prec != precisionOf<Float>())
        throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "createCudaGaugeField: Incompatible precision settings between Displace template and gauge field parameters");
      int X[4], R[4];
      for (int d = 0; d < 4; d++) {
        X[d] = gp.X[d];
        R[d] = 2 * ((comm && (comm->grid[d] > 1 || comm->partitioned[d])) ? 1 : 0);  // exRng[i] = 2 * redundantComms-or-commDimPartitioned, lib/displace.cpp:16
      }
      check(mugiq_hip_alloc_extended_gauge(&ownGauge_, X, R, precisionOf<Float>()));
      const void *links[4] = {lp->gauge[0], lp->gauge[1], lp->gauge[2], lp->gauge[3]};
      const int st = mugiq_hip_create_extended_gauge(&ownGauge_, links, (int)gp.cpu_prec, comm, stream);
      if (st) {
        mugiq_hip_free_extended_gauge(&ownGauge_);
        check(st);
      }
      p.gauge = &ownGauge_;
    }
  }

public:
  Loop_Mugiq(MugiqLoopParam *lp, const std::vector<ColorSpinorField> &eVecs, const std::vector<double> &eVals_sigma,
             const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
    if (eVecs.empty() || eVecs.size() != eVals_sigma.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "Loop_Mugiq: eVecs / eVals_sigma size mismatch");
    checkField<Float, fieldOrder>(&eVecs[0], "Loop_Mugiq");
    CParam c;
    fill(c, lp, comm, stream);
    nEv_ = (int)eVecs.size();
    const int st = mugiq_hip_loop_create(&h_, &c.p, eVecs.data(), eVals_sigma.data(), (int)eVecs.size(), comm, stream);
    if (st) {
      mugiq_hip_free_extended_gauge(&ownGauge_);
      check(st);
    }
  }
  // Two-sided loops (mugiq_hip_loop_create_two_sided): sum_r (1/sigma_r) vL_r^dag G [D^k vR_r] with the left set eVecsLeft and the
  // right (displaced) set eVecsRight, fine-level fields of one geometry, precision and order (the stochastic remainder)
  Loop_Mugiq(MugiqLoopParam *lp, const std::vector<ColorSpinorField> &eVecsLeft, const std::vector<ColorSpinorField> &eVecsRight,
             const std::vector<double> &sigma, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
    if (eVecsRight.empty() || eVecsLeft.size() != eVecsRight.size() || eVecsRight.size() != sigma.size())
      throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "Loop_Mugiq(two-sided): eVecsLeft / eVecsRight / sigma size mismatch");
    checkField<Float, fieldOrder>(&eVecsRight[0], "Loop_Mugiq");
    checkField<Float, fieldOrder>(&eVecsLeft[0], "Loop_Mugiq");
    CParam c;
    fill(c, lp, comm, stream);
    const int st = mugiq_hip_loop_create_two_sided(&h_, &c.p, eVecsLeft.data(), eVecsRight.data(), sigma.data(), (int)eVecsRight.size(),
                                                   comm, stream);
    if (st) {
      mugiq_hip_free_extended_gauge(&ownGauge_);
      check(st);
    }
  }
  // eigsolve->useMGenv && eigsolve->computeCoarse (lib/loop_mugiq.cpp:42,277-319,482): coarse eigenvectors on the coarsest
  // level of the hierarchy + mg_env->transfer[0 .. nCoarseLevels)
  Loop_Mugiq(MugiqLoopParam *lp, const std::vector<MugiqHipCoarseField> &coarseEvecs, const std::vector<double> &eVals_sigma,
             const std::vector<MugiqHipTransfer> &transfers, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
    if (coarseEvecs.empty() || coarseEvecs.size() != eVals_sigma.size() || transfers.empty())
      throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "Loop_Mugiq: coarse eVecs / eVals_sigma / transfer size mismatch");
    if (fieldOrder != FLOAT2_FIELD_ORDER) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "prolongateEvec: Vector prolongation requires fieldOrder = FLOAT2");
    CParam c;
    fill(c, lp, comm, stream);
    const int st = mugiq_hip_loop_create_coarse_levels(&h_, &c.p, coarseEvecs.data(), eVals_sigma.data(), (int)coarseEvecs.size(),
                                                       transfers.data(), (int)transfers.size(), fieldOrder, comm, stream);
    if (st) {
      mugiq_hip_free_extended_gauge(&ownGauge_);
      check(st);
    }
    nEv_ = (int)coarseEvecs.size();
  }
  Loop_Mugiq(const Loop_Mugiq &) = delete;
  Loop_Mugiq &operator=(const Loop_Mugiq &) = delete;
  ~Loop_Mugiq() {
    mugiq_hip_loop_destroy(h_);
    mugiq_hip_free_extended_gauge(&ownGauge_);
  }

  void computeCoarseLoop() { check(mugiq_hip_loop_compute(h_)); }  // lib/loop_mugiq.cpp:439-525
  void writeLoopsHDF5() { check(mugiq_hip_loop_write_hdf5(h_)); }  // lib/loop_mugiq.cpp:668-693

  MugiqHipLoopInfo info() const {
    MugiqHipLoopInfo i;
    check(mugiq_hip_loop_get_info(h_, &i));
    return i;
  }
  MugiqHipLoop *handle() { return h_; }
  // deflateLowModes with this loop's eigenvectors, sigma, comm and stream (one-sided fine-level loops; mugiq_hip_loop_deflate)
  void deflate(const std::vector<ColorSpinorField> &dst, const std::vector<ColorSpinorField> &src, bool gamma5 = true,
               std::vector<std::complex<double>> *overlaps = nullptr) {
    if (src.empty() || dst.size() != src.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "Loop_Mugiq::deflate: size mismatch");
    if (overlaps) overlaps->assign((size_t)nEv_ * src.size(), std::complex<double>(0.0, 0.0));
    check(mugiq_hip_loop_deflate(h_, dst.data(), src.data(), (int)src.size(), gamma5 ? 1 : 0,
                                 overlaps ? reinterpret_cast<double *>(overlaps->data()) : nullptr));
  }
  // deflateLowModesCoarse with this loop's coarse eigenvectors, sigma, transfers, comm and stream (coarse loops; mugiq_hip_loop_deflate_coarse)
  void deflateCoarse(const std::vector<ColorSpinorField> &dst, const std::vector<ColorSpinorField> &src, bool gamma5 = true,
                     std::vector<std::complex<double>> *overlaps = nullptr) {
    if (src.empty() || dst.size() != src.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "Loop_Mugiq::deflateCoarse: size mismatch");
    if (overlaps) overlaps->assign((size_t)nEv_ * src.size(), std::complex<double>(0.0, 0.0));
    check(mugiq_hip_loop_deflate_coarse(h_, dst.data(), src.data(), (int)src.size(), gamma5 ? 1 : 0,
                                        overlaps ? reinterpret_cast<double *>(overlaps->data()) : nullptr));
  }
  int entryKernel(int id) const { return mugiq_hip_loop_get_entry_kernel(h_, id); }  // MUGIQ_HIP_ENTRY_KERNEL_* of the last compute
  const std::complex<Float> *dataPos_d() const { return static_cast<const std::complex<Float> *>(mugiq_hip_loop_data_pos_d(h_)); }
  const std::complex<Float> *dataPos() { return static_cast<const std::complex<Float> *>(mugiq_hip_loop_data_pos_h(h_)); }
  const std::complex<Float> *dataMom_bcast() const { return static_cast<const std::complex<Float> *>(mugiq_hip_loop_data_mom_bcast_h(h_)); }
};

// The kernel form a fused displaced entry runs on, and the geometry of its first launch (mugiq_hip_fused_form; host only)
inline MugiqHipFusedForm fusedForm(const ColorSpinorField &ev, int dispDir, const std::vector<int> &kValues, bool twoSided = false,
                                   bool partitioned = false, bool gaugeGiven = true, int loopPrecision = 0) {
  MugiqHipFusedForm out;
  check(mugiq_hip_fused_form(&ev, twoSided, dispDir, kValues.data(), (int)kValues.size(), partitioned, gaugeGiven, loopPrecision, &out));
  return out;
}

// The kernel forms a finest-level MG transfer runs on, their launch geometry and the level geometry (mugiq_hip_transfer_form; host only)
inline MugiqHipTransferForm transferForm(const MugiqHipTransfer &transfer, int nVec, int fineOrder = 2, int loopPrecision = 0) {
  MugiqHipTransferForm out;
  check(mugiq_hip_transfer_form(&transfer, 0, fineOrder, loopPrecision, nVec, &out));
  return out;
}

// lib/interface_mugiq.cpp:158-172: computeLoop<Float,fieldOrder>(loopParams, eigsolve)
template <typename Float, int fieldOrder>
inline void computeLoop(MugiqLoopParam loopParams, const std::vector<ColorSpinorField> &eVecs, const std::vector<double> &eVals_sigma,
                        const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  Loop_Mugiq<Float, fieldOrder> loop(&loopParams, eVecs, eVals_sigma, comm, stream);
  loop.computeCoarseLoop();
  if (loopParams.writeMomSpaceHDF5 != MUGIQ_BOOL_FALSE || loopParams.writePosSpaceHDF5 != MUGIQ_BOOL_FALSE) loop.writeLoopsHDF5();
  else fprintf(stderr, "computeLoop: Will NOT write output data!\n");  // warningQuda, lib/interface_mugiq.cpp:167
}

}  // namespace mugiq_hip

#endif  // MUGIQ_HIP_OPERATORS_HPP
