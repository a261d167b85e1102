// The five forms of an operator request (MUGIQ_HIP_EIG_OPERATOR_*: M, Mdag, MdagM, MMdag, H = g5 M) and the eigenpair check of
// Eigsolve_Mugiq::computeEvals (lib/eigsolve_mugiq.cpp:289-315), stated once for the operators that serve them: the Wilson / Wilson-clover
// stencil (csrc/wilson.hip), the explicit coarse operator (csrc/coarse_op.hip) and R M P through the transfers (csrc/restrict.hip).
// Host code only.
#pragma once
#include "internal.h"

#include <algorithm>
#include <cmath>

namespace mugiq {

inline bool valid_op(int opType) { return opType >= MUGIQ_HIP_EIG_OPERATOR_M && opType <= MUGIQ_HIP_EIG_OPERATOR_H; }
inline bool normal_op(int opType) { return opType == MUGIQ_HIP_EIG_OPERATOR_MDAGM || opType == MUGIQ_HIP_EIG_OPERATOR_MMDAG; }
inline bool wants_sigma(int opType) { return normal_op(opType) || opType == MUGIQ_HIP_EIG_OPERATOR_H; }
inline double mass_scale(int massNormalization, double kappa) { return massNormalization ? 0.25 / (kappa * kappa) : 1.0; }  // lib/eigsolve_mugiq.cpp:302

// dst_i = scale A src_i, i < n, for a valid form A, out of simple(dst, src, n, dagger, gamma5, scale): dst_i = scale [g5] M^(dag) src_i.
// A normal form is a product of two applications (QUDA's DiracMdagM / DiracMMdag), M first for MdagM and Mdag first for MMdag, through
// the n fields of tmp; the scale goes on the last one
template <typename Simple, typename Field>
int apply_form(int opType, Simple &&simple, const Field *dst, const Field *src, const Field *tmp, int n, double scale) {
  if (!normal_op(opType)) return simple(dst, src, n, opType == MUGIQ_HIP_EIG_OPERATOR_MDAG, opType == MUGIQ_HIP_EIG_OPERATOR_H, scale);
  const int first = opType == MUGIQ_HIP_EIG_OPERATOR_MMDAG;
  if (int st = simple(tmp, src, n, first, 0, 1.0)) return st;
  return simple(dst, tmp, n, !first, 0, scale);
}

// what every eigenpair check asks of its request, behind its own nEv and NULL checks
inline int check_evals_request(int opType, const double *sigma_h, int massNormalization, double kappa, const char *who) {
  MUGIQ_REQUIRE(valid_op(opType), "%s: opType %d is none of M, Mdag, MdagM, MMdag, H", who, opType);
  MUGIQ_REQUIRE(!wants_sigma(opType) || sigma_h != nullptr, "%s: sigma_h is NULL", who);
  MUGIQ_REQUIRE(!massNormalization || kappa != 0.0, "%s: mass normalisation with kappa = 0", who);
  return MUGIQ_HIP_SUCCESS;
}

constexpr int kEvBlock = 8;  // eigenvectors per block of a check: the block of the batched stencils, transfers and reductions

// The check over nEv vectors v, block by block (v0: the first vector of a block of n <= kEvBlock):
//   apply(v0, n)                      w_i = A v_i
//   dot_norm(v0, n, sums)             sums[3 i ..] = (Re, Im <v_i, w_i>, |v_i|^2), on the host
//   residual(v0, n, lambda, sums)     sums[3 i] = |lambda_i v_i - w_i|^2, on the host; lambda: (re, im) of the block.  lambda_h is
//                                     read again once it returns, so it has synchronised
template <typename Apply, typename DotNorm, typename Residual>
int check_eigenpairs(int nEv, int opType, double *lambda_h, double *residual_h, double *sigma_h, Apply &&apply, DotNorm &&dot_norm,
                     Residual &&residual) {
  for (int v0 = 0; v0 < nEv; v0 += kEvBlock) {
    const int n = std::min(kEvBlock, nEv - v0);
    int st;
    double sums[3 * kEvBlock];
    if ((st = apply(v0, n))) return st;
    if ((st = dot_norm(v0, n, sums))) return st;
    for (int i = 0; i < n; i++) {
      const double nrm = std::sqrt(sums[3 * i + 2]);  // lambda = v^dag A v / ||v||   (:303, not ||v||^2)
      lambda_h[2 * (v0 + i)] = sums[3 * i] / nrm;
      lambda_h[2 * (v0 + i) + 1] = sums[3 * i + 1] / nrm;
    }
    if ((st = residual(v0, n, lambda_h + 2 * v0, sums))) return st;
    for (int i = 0; i < n; i++) {
      residual_h[v0 + i] = std::sqrt(sums[3 * i]);  // r = ||lambda v - A v||   (:305-306)
      if (normal_op(opType)) sigma_h[v0 + i] = std::sqrt(lambda_h[2 * (v0 + i)]);  // :311
      else if (opType == MUGIQ_HIP_EIG_OPERATOR_H) sigma_h[v0 + i] = lambda_h[2 * (v0 + i)];
    }
  }
  return MUGIQ_HIP_SUCCESS;
}

}  // namespace mugiq
