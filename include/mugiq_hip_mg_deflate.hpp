// C++ mirror of the deflated coarsest solve of the MG cycle (include/mugiq_hip.h: MugiqHipCoarseDeflation, mugiq_hip_coarse_deflation_build,
// mugiq_hip_coarse_deflate and the *_levels_deflated entry points; csrc/mg_deflate.hip), on top of mugiq_hip_operators.hpp: the space as a
// class, the projection, and the overloads of mgPrecondition / mgPreconditionSloppy / mgSolve / mgSolveMixed that take the space.  A header
// of its own: the program that executes every name of mugiq_hip_operators.hpp on the GPU (tests/cpp/operators.cpp) does not know these
// yet; they are held to the C ABI by a syntax check (tests/test_mg_deflate_cpu.py).
#pragma once
#include <utility>

#include "mugiq_hip_operators.hpp"

namespace mugiq_hip {

// ---- the deflated coarsest solve (csrc/mg_deflate.hip; new): the last coarse level of the four calls above seeded with the lowest
// singular triplets of its operator ----
// The space: W (eigenvectors of MdagM of coarseOp, kept by value as descriptors) and U, whose bodies are the caller's and are filled here
// with M W_n / sigma_n (mugiq_hip_coarse_deflation_build); sigma_n = ||M W_n||.  The bodies must outlive the object
class CoarseDeflation {
public:
  CoarseDeflation(std::vector<MugiqHipCoarseField> W, std::vector<MugiqHipCoarseField> U, const CoarseOperator &coarseOp, const MugiqHipComm *comm = nullptr,
                  void *stream = nullptr)
      : W_(std::move(W)), U_(std::move(U)), sigma_(W_.size(), 0.0) {
    if (W_.empty() || U_.size() != W_.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "CoarseDeflation: size mismatch");
    check(mugiq_hip_coarse_deflation_build(U_.data(), sigma_.data(), W_.data(), (int)W_.size(), coarseOp.desc(), comm, stream));
  }
  const std::vector<double> &sigma() const { return sigma_; }
  MugiqHipCoarseDeflation desc() const { return MugiqHipCoarseDeflation{(int)W_.size(), W_.data(), U_.data(), sigma_.data()}; }

private:
  std::vector<MugiqHipCoarseField> W_, U_;
  std::vector<double> sigma_;
};
// x0_i = sum_n w_n <u_n, b_i> / sigma_n and r0_i = b_i - sum_n u_n <u_n, b_i> (mugiq_hip_coarse_deflate)
inline void coarseDeflate(const std::vector<MugiqHipCoarseField> &x0, const std::vector<MugiqHipCoarseField> &r0, const std::vector<MugiqHipCoarseField> &b,
                          const CoarseDeflation &space, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (b.empty() || x0.size() != b.size() || r0.size() != b.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "coarseDeflate: size mismatch");
  const MugiqHipCoarseDeflation d = space.desc();
  check(mugiq_hip_coarse_deflate(x0.data(), r0.data(), b.data(), (int)b.size(), &d, comm, stream));
}
// the four calls on a hierarchy with a space on its last level (the *_levels_deflated entry points)
inline void mgPrecondition(const std::vector<ColorSpinorField> &z, const std::vector<ColorSpinorField> &r, const GaugeField &gauge,
                           const MugiqHipCloverField *clover, double kappa, const std::vector<MugiqHipTransfer> &transfers,
                           const std::vector<MugiqHipCoarseOperator> &coarseOps, const std::vector<MgSolveParam> &params, const CoarseDeflation &deflation,
                           const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (r.empty() || z.size() != r.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgPrecondition: size mismatch");
  const int L = detail::mgLevels(transfers, coarseOps, params, "mgPrecondition");
  const MugiqHipCoarseDeflation d = deflation.desc();
  check(mugiq_hip_mg_precondition_levels_deflated(z.data(), r.data(), (int)r.size(), &gauge, clover, kappa, transfers.data(), coarseOps.data(), L, params.data(),
                                                  &d, comm, stream));
}
inline void mgPreconditionSloppy(const std::vector<ColorSpinorField> &z, const std::vector<ColorSpinorField> &r, const GaugeField &gauge,
                                 const MugiqHipCloverField *clover, double kappa, const std::vector<MugiqHipTransfer> &transfers,
                                 const std::vector<MugiqHipCoarseOperator> &coarseOps, const std::vector<MgSolveParam> &params,
                                 const CoarseDeflation &deflation, const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (r.empty() || z.size() != r.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgPreconditionSloppy: size mismatch");
  const int L = detail::mgLevels(transfers, coarseOps, params, "mgPreconditionSloppy");
  const MugiqHipCoarseDeflation d = deflation.desc();
  check(mugiq_hip_mg_precondition_sloppy_levels_deflated(z.data(), r.data(), (int)r.size(), &gauge, clover, kappa, transfers.data(), coarseOps.data(), L,
                                                         params.data(), &d, comm, stream));
}
inline bool mgSolve(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, const GaugeField &gauge,
                    const MugiqHipCloverField *clover, double kappa, const std::vector<MugiqHipTransfer> &transfers,
                    const std::vector<MugiqHipCoarseOperator> &coarseOps, const std::vector<MgSolveParam> &params, const CoarseDeflation &deflation,
                    std::vector<int> &iters, std::vector<double> &relres, std::vector<std::vector<double>> *history = nullptr, int *hostReads = nullptr,
                    const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (b.empty() || x.size() != b.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgSolve: size mismatch");
  const int L = detail::mgLevels(transfers, coarseOps, params, "mgSolve");
  const MugiqHipCoarseDeflation d = deflation.desc();
  int stride;
  std::vector<double> hist = detail::mgOutputs(b.size(), params[0].maxIter, history != nullptr, iters, relres, &stride);
  const int st = mugiq_hip_mg_solve_levels_deflated(x.data(), b.data(), (int)b.size(), &gauge, clover, kappa, transfers.data(), coarseOps.data(), L,
                                                    params.data(), &d, iters.data(), relres.data(), history ? hist.data() : nullptr, stride, hostReads, comm,
                                                    stream);
  return detail::mgHistory(st, hist, stride, iters, history);
}
inline bool mgSolveMixed(const std::vector<ColorSpinorField> &x, const std::vector<ColorSpinorField> &b, const GaugeField &gauge,
                         const MugiqHipCloverField *clover, double kappa, const GaugeField *gaugeSloppy, const MugiqHipCloverField *cloverSloppy,
                         const std::vector<MugiqHipTransfer> &transfersSloppy, const std::vector<MugiqHipCoarseOperator> &coarseOpsSloppy,
                         const std::vector<MgSolveParam> &params, const CoarseDeflation &deflationSloppy, std::vector<int> &iters,
                         std::vector<double> &relres, std::vector<std::vector<double>> *history = nullptr, int *hostReads = nullptr,
                         const MugiqHipComm *comm = nullptr, void *stream = nullptr) {
  if (b.empty() || x.size() != b.size()) throw Error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "mgSolveMixed: size mismatch");
  const int L = detail::mgLevels(transfersSloppy, coarseOpsSloppy, params, "mgSolveMixed");
  const MugiqHipCoarseDeflation d = deflationSloppy.desc();
  int stride;
  std::vector<double> hist = detail::mgOutputs(b.size(), params[0].maxIter, history != nullptr, iters, relres, &stride);
  const int st = mugiq_hip_mg_solve_mixed_levels_deflated(x.data(), b.data(), (int)b.size(), &gauge, clover, kappa, gaugeSloppy, cloverSloppy,
                                                          transfersSloppy.data(), coarseOpsSloppy.data(), L, params.data(), &d, iters.data(), relres.data(),
                                                          history ? hist.data() : nullptr, stride, hostReads, comm, stream);
  return detail::mgHistory(st, hist, stride, iters, history);
}

}  // namespace mugiq_hip
