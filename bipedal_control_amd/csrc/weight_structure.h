// The structural zeros of the cost weights Q and R, found once when the model is created.  Host-only on purpose - plain C++, no HIP header, no
// kernel header - so that tests/test_weight_structure.py compiles it alone.
// The weights are constants of the model and almost entirely zeros (Q is diagonal, R has its diagonal force entries and one dense block per leg:
// at most 6 non-zeros per row on the robots of the reference).  The hot kernels form their gradient sums sum_r W[c][r] d[r] over the non-zero
// columns of row c only.  A skipped term is a product with an exact zero: adding it changes no bit of a finite sum that starts from +0.0, and the
// remaining terms keep their order (ascending r), so the results are the bits of the dense sums.
#pragma once
#include <cmath>

namespace bpmpc {

constexpr int kMaxWeightTerms = 8;      // non-zeros per row up to which the compact form exists
constexpr int kWeightDim = 24;          // rows / columns of a weight at most (kMaxState of robot_model.h; device_model.h asserts it)
constexpr int kWeightRowStride = 2 * kWeightDim * kWeightDim;   // a per-problem weight row: Q (nx x nx, stride nx) then R (nu x nu, stride nu), the rest 0 (BPMPC_SOLVER_WEIGHT_STRIDE)

// Term-major lists: val[j][c], idx[j][c] = the j-th non-zero entry of row c and its column, columns ascending; lanes on consecutive c read
// consecutive words.  A row with fewer than K entries is padded with the pair (0.0, c): a term that adds +0.0.
struct WeightTerms {
  double val[kMaxWeightTerms][kWeightDim];
  unsigned char idx[kMaxWeightTerms][kWeightDim];
};

struct WeightStructure {
  WeightTerms q, r;
  double q_diag[kWeightDim];            // the diagonal of Q
  int k_q, k_r;                         // largest number of non-zeros over the rows of Q / of R (counted beyond kMaxWeightTerms too)
  int q_diagonal;                       // 1: every off-diagonal entry of Q is zero
  int compact;                          // 1: both lists exist (k_q, k_r <= kMaxWeightTerms); 0: the kernels run their dense sums
};

// Lists of one n x n weight (row major, stride n); returns the largest number of non-zeros of a row.  An entry equal to zero of either sign counts
// as zero.  Rows beyond kMaxWeightTerms entries keep their first kMaxWeightTerms (the caller then does not use the lists).
inline int find_weight_terms(const double* w, int n, WeightTerms& t) {
  int kmax = 0;
  for (int j = 0; j < kMaxWeightTerms; ++j)
    for (int c = 0; c < kWeightDim; ++c) { t.val[j][c] = 0.0; t.idx[j][c] = (unsigned char)(c < n ? c : 0); }
  if (n > kWeightDim) return n;         // no lists (the caller runs dense)
  for (int c = 0; c < n; ++c) {
    int k = 0;
    for (int r = 0; r < n; ++r) {
      const double v = w[c * n + r];
      if (v == 0.0) continue;           // (true for -0.0 as well)
      if (k < kMaxWeightTerms) { t.val[k][c] = v; t.idx[k][c] = (unsigned char)r; }
      ++k;
    }
    if (k > kmax) kmax = k;
  }
  return kmax;
}

// Q: nx x nx, R: nu x nu, both row major with their own dimension as the stride (DeviceModel::Q, R)
inline WeightStructure find_weight_structure(const double* Q, int nx, const double* R, int nu) {
  WeightStructure s;
  s.k_q = find_weight_terms(Q, nx, s.q);
  s.k_r = find_weight_terms(R, nu, s.r);
  s.q_diagonal = 1;
  for (int c = 0; c < kWeightDim; ++c) s.q_diag[c] = c < nx ? Q[c * nx + c] : 0.0;
  for (int c = 0; c < nx; ++c)
    for (int r = 0; r < nx; ++r)
      if (r != c && Q[c * nx + r] != 0.0) s.q_diagonal = 0;
  s.compact = (nx <= kWeightDim && nu <= kWeightDim && s.k_q <= kMaxWeightTerms && s.k_r <= kMaxWeightTerms) ? 1 : 0;
  return s;
}

// ---- per-problem weight rows (bpmpc_solver_set_weights): what a host row must satisfy before it may stand in for the model's weights
// A row is Q (nx x nx, stride nx) followed by R (nu x nu, stride nu).  The PATTERN rule - no non-zero where the model's Q or R has a structural
// zero - is what keeps everything derived from the model's pattern valid for every row: the index lists above, q_diagonal (the change of variables
// builds [Q | q | 0] from the diagonal), and the block-diagonal test of R behind the structured change of variables.  The others are what the
// solve needs of any cost: finite, symmetric (to kWeightSymmetryTol relative: the model's own R = J^T R_v J is symmetric up to rounding only),
// Q positive semidefinite (a diagonal Q: no negative diagonal entry), R positive definite (semidefinite where the model's own R is only that).
enum class WeightFault { None = 0, NotFinite, NotSymmetric, OffPattern, QNegativeDiagonal, QNotPsd, RNotPositiveDefinite };
struct WeightVerdict {
  WeightFault fault;
  char matrix;          // 'Q' or 'R'
  int row, col;         // the entry (the pivot for the definiteness faults)
};
constexpr double kWeightSymmetryTol = 1e-9;

inline const char* weight_fault_text(WeightFault f) {
  switch (f) {
    case WeightFault::None: return "accepted";
    case WeightFault::NotFinite: return "is not finite";
    case WeightFault::NotSymmetric: return "differs from its transposed entry: the weight is not symmetric";
    case WeightFault::OffPattern: return "is non-zero where the model's weight has a structural zero";
    case WeightFault::QNegativeDiagonal: return "is a negative diagonal entry of Q";
    case WeightFault::QNotPsd: return "is a negative pivot: Q is not positive semidefinite";
    case WeightFault::RNotPositiveDefinite: return "is a pivot that is not positive: R is not positive definite (as far as the model's R is)";
  }
  return "?";
}

// n x n, stride n: 0 when every off-diagonal non-zero of w lies on a non-zero of the model's weight m, else 1 with the first entry off the pattern
inline int weight_off_pattern(const double* w, const double* m, int n, int* row, int* col) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      if (m[i * n + j] == 0.0 && w[i * n + j] != 0.0) { *row = i; *col = j; return 1; }
  return 0;
}

// Cholesky with diagonal pivoting on a copy of the symmetric n x n weight w (n <= kWeightDim).  strict: every pivot must be positive (positive
// definite); else a pivot may vanish, and once the largest remaining one has, the remaining block must have vanished with it (positive
// semidefinite).  A pivot counts as zero within n * n * 2^-52 * the largest diagonal entry (what n elimination steps leave of an exact zero).
// Returns 1 and the failing pivot's index, or 0.
inline int weight_not_definite(const double* w, int n, bool strict, int* pivot) {
  double a[kWeightDim][kWeightDim];
  int perm[kWeightDim];
  double dmax = 0.0;
  for (int i = 0; i < n; ++i) {
    perm[i] = i;
    for (int j = 0; j < n; ++j) a[i][j] = 0.5 * (w[i * n + j] + w[j * n + i]);
    if (std::fabs(a[i][i]) > dmax) dmax = std::fabs(a[i][i]);
  }
  const double tol = n * n * 2.220446049250313e-16 * dmax;
  for (int k = 0; k < n; ++k) {
    int p = k;
    for (int i = k + 1; i < n; ++i)
      if (a[i][i] > a[p][p]) p = i;
    if (a[p][p] <= tol) {
      if (strict) { *pivot = perm[p]; return 1; }
      // semidefinite: nothing of the remaining block may be left, neither a negative diagonal entry nor an off-diagonal one
      for (int i = k; i < n; ++i)
        for (int j = k; j < n; ++j)
          if ((i == j && a[i][i] < -tol) || (i != j && std::fabs(a[i][j]) > tol)) { *pivot = perm[i]; return 1; }
      return 0;
    }
    if (p != k) {
      for (int j = 0; j < n; ++j) { const double t = a[k][j]; a[k][j] = a[p][j]; a[p][j] = t; }
      for (int i = 0; i < n; ++i) { const double t = a[i][k]; a[i][k] = a[i][p]; a[i][p] = t; }
      const int t = perm[k]; perm[k] = perm[p]; perm[p] = t;
    }
    const double d = a[k][k];
    for (int i = k + 1; i < n; ++i) {
      const double l = a[i][k] / d;
      for (int j = k + 1; j < n; ++j) a[i][j] -= l * a[k][j];
    }
  }
  return 0;
}

// The whole check of one host row against the model's Q (nx x nx) and R (nu x nu); the first fault in the order of the enumeration
inline WeightVerdict check_weight_row(const double* row, const double* Qm, int nx, const double* Rm, int nu) {
  const double* w[2] = {row, row + nx * nx};
  const double* m[2] = {Qm, Rm};
  const int n[2] = {nx, nu};
  const char name[2] = {'Q', 'R'};
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < n[t] * n[t]; ++i)
      if (!std::isfinite(w[t][i])) return {WeightFault::NotFinite, name[t], i / n[t], i % n[t]};
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < n[t]; ++i)
      for (int j = i + 1; j < n[t]; ++j) {
        const double a = w[t][i * n[t] + j], b = w[t][j * n[t] + i];
        const double scale = std::fabs(a) > std::fabs(b) ? std::fabs(a) : std::fabs(b);
        if (std::fabs(a - b) > kWeightSymmetryTol * scale) return {WeightFault::NotSymmetric, name[t], i, j};
      }
  for (int t = 0; t < 2; ++t) {
    int i = 0, j = 0;
    if (weight_off_pattern(w[t], m[t], n[t], &i, &j)) return {WeightFault::OffPattern, name[t], i, j};
  }
  bool q_diagonal = true;
  for (int i = 0; i < nx; ++i)
    for (int j = 0; j < nx; ++j)
      if (i != j && Qm[i * nx + j] != 0.0) q_diagonal = false;
  int p = 0;
  if (q_diagonal) {
    for (int i = 0; i < nx; ++i)
      if (row[i * nx + i] < 0.0) return {WeightFault::QNegativeDiagonal, 'Q', i, i};
  } else if (weight_not_definite(row, nx, false, &p)) {
    return {WeightFault::QNotPsd, 'Q', p, p};
  }
  // R: positive definite - where the model's own R is.  With six joints per leg J^T R_v J is only positive SEMIdefinite (the two contact points of a
  // rigid foot keep their distance: J has rank 10 of 12), and a row is then held to what the model's row satisfies.
  const bool r_strict = !weight_not_definite(Rm, nu, true, &p);
  if (weight_not_definite(row + nx * nx, nu, r_strict, &p)) return {WeightFault::RNotPositiveDefinite, 'R', p, p};
  return {WeightFault::None, 'Q', 0, 0};
}

}  // namespace bpmpc
