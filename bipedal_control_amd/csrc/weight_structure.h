// The structural zeros of the cost weights Q and R, found once when the model is created.  Host-only on purpose - plain C++, no HIP header, no
// kernel header - so that tests/test_weight_structure.py compiles it alone.
// The weights are constants of the model and almost entirely zeros (Q is diagonal, R has its diagonal force entries and one dense block per leg:
// at most 6 non-zeros per row on the robots of the reference).  The hot kernels form their gradient sums sum_r W[c][r] d[r] over the non-zero
// columns of row c only.  A skipped term is a product with an exact zero: adding it changes no bit of a finite sum that starts from +0.0, and the
// remaining terms keep their order (ascending r), so the results are the bits of the dense sums.
#pragma once

namespace bpmpc {

constexpr int kMaxWeightTerms = 8;      // non-zeros per row up to which the compact form exists
constexpr int kWeightDim = 24;          // rows / columns of a weight at most (kMaxState of robot_model.h; device_model.h asserts it)

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

}  // namespace bpmpc
