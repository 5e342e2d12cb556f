// The fp64 MFMA product kernel of csrc/linear_svm.hip as other sources may use it: one tile kernel, its epilogue chosen at run time.
#pragma once
#include "common.h"

namespace hsefr {

// out[i][j] = exp(-gamma max(0, norm_a[i] + norm_b[j] - 2 <a_i, b_j>)) in fp64 (libsvm's own formula of the RBF kernel), out [ma, mb]
// with row stride ldo; a [ma, d] and b [mb, d] fp32 row-major, norm_a / norm_b their rows' squared norms in fp64.  training (a == b): the
// matrix as libsvm's solver holds it -- every value rounded to fp32, its Qfloat, and out[i][i] = 1 exactly.  The sum over d of one entry
// has the same shape wherever its tile lies.
int svm_rbf_kernel_matrix(const float* a, int ma, const double* norm_a, const float* b, int mb, const double* norm_b, int d, double gamma,
                          double* out, long long ldo, int training, const char* what, hipStream_t s);

}  // namespace hsefr
