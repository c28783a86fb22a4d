// trm_launch_average.hip -- k_accumulate (trm_average.hpp): the time averages of every program that does not accumulate in its own
// launch, one launch after every step launch covering every open accumulator.
#include "trm_host.hpp"

namespace trm {

// blockIdx.y: the entry; grid-stride over its elements.  Bandwidth-bound: one read of the field, a read-modify-write of the sum.
template <class NF> __global__ void __launch_bounds__(256) k_accumulate(AccumBatch b) {
    const AccumEntry& en = b.e[blockIdx.y];
    const long long n = en.n;
    const long long stride = (long long)gridDim.x * blockDim.x;
    double* sum = en.sum;
    if (en.src_double) {
        const double* src = (const double*)en.src;
        for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride)
            if (en.pitch == 1 || (int)(e % en.pitch) < en.nz) sum[e] = sum[e] + src[e];
    } else {
        const NF* src = (const NF*)en.src;
        const double w = b.w;
        for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride)
            if (en.pitch == 1 || (int)(e % en.pitch) < en.nz) sum[e] = sum[e] + w * (double)src[e];
    }
}

}  // namespace trm

namespace trmh {

template <class NF> int AverageLaunch<NF>::accumulate(trm_ctx* c, const AccumBatch& b) {
    if (b.count <= 0) return TRM_OK;
    long long most = 0;
    for (int j = 0; j < b.count; ++j) most = std::max(most, b.e[j].n);
    // (enough workgroups to fill the device on the largest entry, never more than it has elements for)
    const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((most + 255) / 256, 2048));
    hipLaunchKernelGGL((k_accumulate<NF>), dim3(gx, (unsigned)b.count, 1), dim3(256), 0, c->stream, b);
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

template struct AverageLaunch<double>;
template struct AverageLaunch<float>;

}  // namespace trmh
