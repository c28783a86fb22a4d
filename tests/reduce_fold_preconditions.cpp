// The host side of the two-operand folds of TRM_REDUCE_MIN / TRM_REDUCE_MAX (trm_reduce_fold.hpp: the same functions fold the block
// partials of k_reduce_rows in reduce_impl and the shards in trm_reduce_global_all): Julia's Base.minimum / maximum on NaN, the
// infinities and zeros of both signs, in both operand orders and through a fold from the identity in every order of the operands.
// Built with the host sanitizers and run by `make -C terrarium.jl_amd/csrc check-preconditions` (cross-compiles; runs without a GPU).
#include "trm_reduce_fold.hpp"
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <vector>

using trmh::nan_max;
using trmh::nan_min;

static bool same(double a, double b) { return (a != a && b != b) || (a == b && std::signbit(a) == std::signbit(b)); }

int main() {
    const double inf = HUGE_VAL, nan = std::nan(""), pz = 0.0, nz = -0.0;
    // zeros: the minimum is the negative one, the maximum the positive one, whichever comes first
    assert(same(nan_min(pz, nz), nz) && same(nan_min(nz, pz), nz) && same(nan_min(pz, pz), pz) && same(nan_min(nz, nz), nz));
    assert(same(nan_max(pz, nz), pz) && same(nan_max(nz, pz), pz) && same(nan_max(pz, pz), pz) && same(nan_max(nz, nz), nz));
    // NaN wins against everything, the identities and the infinities included
    for (double x : {nan, pz, nz, 1.0, -1.0, inf, -inf}) {
        assert(std::isnan(nan_min(nan, x)) && std::isnan(nan_min(x, nan)));
        assert(std::isnan(nan_max(nan, x)) && std::isnan(nan_max(x, nan)));
    }
    // ordinary operands and infinities
    assert(nan_min(1.0, 2.0) == 1.0 && nan_min(2.0, 1.0) == 1.0 && nan_max(1.0, 2.0) == 2.0 && nan_max(2.0, 1.0) == 2.0);
    assert(nan_min(-inf, inf) == -inf && nan_min(inf, -inf) == -inf && nan_max(-inf, inf) == inf && nan_max(inf, -inf) == inf);
    assert(nan_min(inf, inf) == inf && nan_max(-inf, -inf) == -inf && nan_min(inf, 3.0) == 3.0 && nan_max(-inf, 3.0) == 3.0);
    assert(same(nan_min(5e-324, nz), nz) && same(nan_max(-5e-324, pz), pz) && same(nan_min(-5e-324, nz), -5e-324));
    // a fold from the identity, as the kernel and reduce_impl run it, over every order of the operands
    const double with_max[4] = {pz, nz, pz, 2.0}, with_min[4] = {nz, pz, nz, -2.0};
    std::vector<int> order = {0, 1, 2, 3};
    do {
        double lo = HUGE_VAL, hi = -HUGE_VAL, lo2 = HUGE_VAL, hi2 = -HUGE_VAL;
        for (int j : order) {
            lo = nan_min(lo, with_max[j]); hi = nan_max(hi, with_max[j]);
            lo2 = nan_min(lo2, with_min[j]); hi2 = nan_max(hi2, with_min[j]);
        }
        assert(same(lo, nz) && hi == 2.0 && lo2 == -2.0 && same(hi2, pz));
    } while (std::next_permutation(order.begin(), order.end()));
    std::puts("reduce fold preconditions ok");
    return 0;
}
