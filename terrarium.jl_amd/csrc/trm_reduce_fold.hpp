// trm_reduce_fold.hpp -- the two-operand folds of TRM_REDUCE_MIN / TRM_REDUCE_MAX, shared by the device kernel (k_reduce_rows), the host
// fold of its block partials (reduce_impl), the host fold of the shards (trm_reduce_global_all without communicators) and the
// stand-alone host check tests/reduce_fold_preconditions.cpp.
#pragma once
#include <hip/hip_runtime.h>

namespace trmh {
// minimum / maximum as Julia's Base.minimum / maximum: a NaN anywhere gives NaN, and of two zeros that compare equal the minimum is
// the negative one, the maximum the positive one (minimum([0.0, -0.0]) === -0.0, maximum([-0.0, 0.0]) === 0.0) -- in whatever order
// the operands arrive, so the sign of a zero result does not depend on the fold order.
__host__ __device__ inline double nan_min(double a, double b) {
    if (a != a || b != b) return a + b;
    if (a < b) return a;
    if (b < a) return b;
    return __builtin_signbit(a) ? a : b;
}
__host__ __device__ inline double nan_max(double a, double b) {
    if (a != a || b != b) return a + b;
    if (a > b) return a;
    if (b > a) return b;
    return __builtin_signbit(a) ? b : a;
}
}  // namespace trmh
