// Dense Hermitian algebra on the host for the coarse-grid eigensolver (csrc/coarse_eig.hip): the eigendecomposition of the Rayleigh-Ritz
// matrix and the Cholesky factor and triangular inverse of a Gram matrix, n <= 512.  No LAPACK: Householder tridiagonalisation with the
// unitary accumulated, a diagonal phase matrix that makes the tridiagonal real, and the implicit-shift QL iteration on it (EISPACK's
// htridi / tql2 in one piece).  Every step is a unitary similarity, so the result is backward stable: |H Z - Z Theta| and |Z^dag Z - 1|
// are a modest multiple of n eps |H| whatever the spectrum (clusters and repeated eigenvalues included).
// Matrices are row-major arrays of n x n complex numbers, (re, im) interleaved.  Contracts: include/mugiq_hip.h.
#include "internal.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <numeric>
#include <vector>

namespace mugiq {
namespace {

typedef std::complex<double> C;
constexpr int kDenseMax = 512;

// Householder: H -> T = Q^dag H Q real tridiagonal (d, e: e[i] = T[i+1][i], e[n-1] = 0), Qt[j][.] = column j of Q
void tridiagonalize(int n, std::vector<C> &A, std::vector<double> &d, std::vector<double> &e, std::vector<C> &Qt) {
  std::vector<C> v(n), p(n), w(n), sub(n, C(0.0, 0.0));
  std::vector<double> beta(n, 0.0);  // reflector k is 1 - beta v v^dag, v kept in column k of A below the subdiagonal and v[k+1] apart
  std::vector<C> head(n, C(0.0, 0.0));
  for (int k = 0; k + 2 < n; k++) {
    double tail2 = 0.0;
    for (int i = k + 2; i < n; i++) tail2 += std::norm(A[(size_t)i * n + k]);
    const C x0 = A[(size_t)(k + 1) * n + k];
    if (tail2 == 0.0) {  // nothing to annihilate
      sub[k] = x0;
      continue;
    }
    const double nx = std::sqrt(std::norm(x0) + tail2);
    const C ph = std::abs(x0) > 0.0 ? x0 / std::abs(x0) : C(1.0, 0.0);
    const C alpha = -ph * nx;
    // v = x - alpha e_1, beta = 2 / |v|^2
    v[k + 1] = x0 - alpha;
    for (int i = k + 2; i < n; i++) v[i] = A[(size_t)i * n + k];
    const double v2 = std::norm(v[k + 1]) + tail2;
    const double b = 2.0 / v2;
    // p = b A22 v, w = p - (b/2) (v^dag p) v, A22 -= v w^dag + w v^dag
    for (int i = k + 1; i < n; i++) {
      C s(0.0, 0.0);
      for (int j = k + 1; j < n; j++) s += A[(size_t)i * n + j] * v[j];
      p[i] = b * s;
    }
    C vp(0.0, 0.0);
    for (int i = k + 1; i < n; i++) vp += std::conj(v[i]) * p[i];
    for (int i = k + 1; i < n; i++) w[i] = p[i] - (0.5 * b) * vp * v[i];
    for (int i = k + 1; i < n; i++)
      for (int j = k + 1; j < n; j++) A[(size_t)i * n + j] -= v[i] * std::conj(w[j]) + w[i] * std::conj(v[j]);
    sub[k] = alpha;
    beta[k] = b;
    head[k] = v[k + 1];
    for (int i = k + 2; i < n; i++) A[(size_t)i * n + k] = v[i];
  }
  if (n >= 2) sub[n - 2] = A[(size_t)(n - 1) * n + (n - 2)];
  // Q = H_0 H_1 ... H_{n-3}, built from the right; row r of Qt is column r of Q
  std::fill(Qt.begin(), Qt.end(), C(0.0, 0.0));
  for (int i = 0; i < n; i++) Qt[(size_t)i * n + i] = 1.0;
  for (int k = n - 3; k >= 0; k--) {
    if (beta[k] == 0.0) continue;
    v[k + 1] = head[k];
    for (int i = k + 2; i < n; i++) v[i] = A[(size_t)i * n + k];
    // Q <- H_k Q: every column c of Q (row c of Qt) -= beta v (v^dag column)
    for (int c = k + 1; c < n; c++) {
      C *col = &Qt[(size_t)c * n];
      C s(0.0, 0.0);
      for (int i = k + 1; i < n; i++) s += std::conj(v[i]) * col[i];
      s *= beta[k];
      for (int i = k + 1; i < n; i++) col[i] -= s * v[i];
    }
  }
  // T_c has the complex subdiagonal sub; with D = diag(ph_j), ph_0 = 1, ph_{j+1} = ph_j sub_j / |sub_j|, D^dag T_c D is real
  C ph(1.0, 0.0);
  for (int j = 0; j < n; j++) {
    d[j] = A[(size_t)j * n + j].real();
    if (j > 0) {
      const double a = std::abs(sub[j - 1]);
      if (a > 0.0) ph *= sub[j - 1] / a;
      ph /= std::abs(ph);  // keep the modulus from drifting
      e[j - 1] = a;
      C *col = &Qt[(size_t)j * n];
      for (int i = 0; i < n; i++) col[i] *= ph;
    }
  }
  e[n - 1] = 0.0;
}

// implicit-shift QL on (d, e), the rotations applied to the rows of Zt (columns of Z).  false: no convergence within 60 sweeps of one value
bool ql_implicit(int n, std::vector<double> &d, std::vector<double> &e, std::vector<C> &Zt) {
  const double eps = 2.220446049250313e-16;
  for (int l = 0; l < n; l++) {
    int iter = 0, m;
    do {
      for (m = l; m < n - 1; m++) {
        const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
        if (std::fabs(e[m]) <= eps * dd) break;
      }
      if (m != l) {
        if (iter++ == 60) return false;
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
        double r = std::hypot(g, 1.0);
        g = d[m] - d[l] + e[l] / (g + std::copysign(r, g));
        double s = 1.0, c = 1.0, p = 0.0;
        int i;
        for (i = m - 1; i >= l; i--) {
          double f = s * e[i];
          const double b = c * e[i];
          e[i + 1] = (r = std::hypot(f, g));
          if (r == 0.0) {
            d[i + 1] -= p;
            e[m] = 0.0;
            break;
          }
          s = f / r;
          c = g / r;
          g = d[i + 1] - p;
          r = (d[i] - g) * s + 2.0 * c * b;
          d[i + 1] = g + (p = s * r);
          g = c * r - b;
          C *z0 = &Zt[(size_t)i * n], *z1 = &Zt[(size_t)(i + 1) * n];
          for (int k = 0; k < n; k++) {
            const C f1 = z1[k];
            z1[k] = s * z0[k] + c * f1;
            z0[k] = c * z0[k] - s * f1;
          }
        }
        if (r == 0.0 && i >= l) continue;
        d[l] -= p;
        e[l] = g;
        e[m] = 0.0;
      }
    } while (m != l);
  }
  return true;
}

}  // namespace

// for csrc/coarse_eig.hip, behind the checks of the exported calls
int hermitian_eigh(int n, const double *H, double *theta, double *Z, const char *who) {
  std::vector<C> A((size_t)n * n), Qt((size_t)n * n);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      const C a(H[2 * ((size_t)i * n + j)], H[2 * ((size_t)i * n + j) + 1]), b(H[2 * ((size_t)j * n + i)], H[2 * ((size_t)j * n + i) + 1]);
      const C h = 0.5 * (a + std::conj(b));
      if (!std::isfinite(h.real()) || !std::isfinite(h.imag())) return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: H[%d][%d] is not finite", who, i, j);
      A[(size_t)i * n + j] = h;
    }
  std::vector<double> d(n), e(n);
  tridiagonalize(n, A, d, e, Qt);
  if (!ql_implicit(n, d, e, Qt)) return set_error(MUGIQ_HIP_ERROR_NOT_CONVERGED, "%s: the QL iteration did not converge", who);
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return d[a] < d[b]; });
  for (int j = 0; j < n; j++) {
    theta[j] = d[order[j]];
    const C *col = &Qt[(size_t)order[j] * n];
    for (int i = 0; i < n; i++) {
      Z[2 * ((size_t)i * n + j)] = col[i].real();
      Z[2 * ((size_t)i * n + j) + 1] = col[i].imag();
    }
  }
  return MUGIQ_HIP_SUCCESS;
}

// G = R^dag R column by column; status 1 at the first pivot <= rankTol max diag G (or not finite), *badPivot = its index, *pivot its value
int cholesky_upper(int n, const double *G, double *R, double rankTol, int *badPivot, double *pivot, const char *who) {
  const C *g = reinterpret_cast<const C *>(G);
  C *r = reinterpret_cast<C *>(R);
  std::fill(r, r + (size_t)n * n, C(0.0, 0.0));
  double big = 0.0;
  for (int j = 0; j < n; j++) big = std::max(big, g[(size_t)j * n + j].real());
  const double floor = rankTol * big;
  if (badPivot) *badPivot = -1;
  for (int j = 0; j < n; j++) {
    for (int i = 0; i < j; i++) {
      C s = g[(size_t)i * n + j];
      for (int k = 0; k < i; k++) s -= std::conj(r[(size_t)k * n + i]) * r[(size_t)k * n + j];
      r[(size_t)i * n + j] = s / r[(size_t)i * n + i].real();
    }
    double piv = g[(size_t)j * n + j].real();
    for (int k = 0; k < j; k++) piv -= std::norm(r[(size_t)k * n + j]);
    if (!(piv > floor) || !std::isfinite(piv)) {
      if (badPivot) *badPivot = j;
      if (pivot) *pivot = piv;
      return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: pivot %d of the Cholesky factorisation is %.3e <= rankTol %.3e x max diag %.3e: the columns are dependent", who,
                       j, piv, rankTol, big);
    }
    r[(size_t)j * n + j] = std::sqrt(piv);
  }
  return MUGIQ_HIP_SUCCESS;
}

int upper_inverse(int n, const double *R, double *Rinv, const char *who) {
  const C *r = reinterpret_cast<const C *>(R);
  C *x = reinterpret_cast<C *>(Rinv);
  for (int j = 0; j < n; j++) {
    const C dj = r[(size_t)j * n + j];
    if (dj == C(0.0, 0.0) || !std::isfinite(dj.real()) || !std::isfinite(dj.imag()))
      return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: R[%d][%d] is zero or not finite", who, j, j);
  }
  std::fill(x, x + (size_t)n * n, C(0.0, 0.0));
  for (int j = 0; j < n; j++) {
    x[(size_t)j * n + j] = 1.0 / r[(size_t)j * n + j];
    for (int i = j - 1; i >= 0; i--) {
      C s(0.0, 0.0);
      for (int k = i + 1; k <= j; k++) s += r[(size_t)i * n + k] * x[(size_t)k * n + j];
      x[(size_t)i * n + j] = -s / r[(size_t)i * n + i];
    }
  }
  return MUGIQ_HIP_SUCCESS;
}

}  // namespace mugiq

using namespace mugiq;

extern "C" {

int mugiq_hip_hermitian_eigh(int n, const double *H, double *theta, double *Z) {
  const char *who = "hermitianEigh";
  MUGIQ_REQUIRE(H != nullptr && theta != nullptr && Z != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(n >= 1 && n <= kDenseMax, "%s: n = %d must be in [1, %d]", who, n, kDenseMax);
  return hermitian_eigh(n, H, theta, Z, who);
}

int mugiq_hip_cholesky_upper(int n, const double *G, double *R, double rankTol, int *badPivot, double *pivot) {
  const char *who = "choleskyUpper";
  MUGIQ_REQUIRE(G != nullptr && R != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(n >= 1 && n <= kDenseMax, "%s: n = %d must be in [1, %d]", who, n, kDenseMax);
  MUGIQ_REQUIRE(rankTol >= 0.0 && rankTol <= 1.0, "%s: rankTol = %g must be in [0, 1]", who, rankTol);
  return cholesky_upper(n, G, R, rankTol, badPivot, pivot, who);
}

int mugiq_hip_upper_triangular_inverse(int n, const double *R, double *Rinv) {
  const char *who = "upperTriangularInverse";
  MUGIQ_REQUIRE(R != nullptr && Rinv != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(n >= 1 && n <= kDenseMax, "%s: n = %d must be in [1, %d]", who, n, kDenseMax);
  return upper_inverse(n, R, Rinv, who);
}

}  // extern "C"
