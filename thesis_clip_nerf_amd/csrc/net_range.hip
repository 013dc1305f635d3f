// Weight range of one Keras-order MLP (mvnerf_net_range): what decides whether the fp16 two-piece field kernel may run it.
//   out2[0] = max |w| over what mvnerf_pack_net_split cuts into 16-bit weight pieces: the 379 rows of W0 and the 12 hidden kernels
//             (not the biases, not the read-out: they stay fp32);
//   out2[1] = max |.| over all 247300 variables.
// Both as the bit pattern of the non-negative float under an unsigned max (the convention of the field kernel's range status): a NaN
// variable leaves a NaN, infinity leaves infinity.
#include <hip/hip_runtime.h>

#include "mvnerf_kernels.h"
#include "mvnerf_math.h"

namespace mvnerf {

namespace {

constexpr int kNetVars = kKerasBr + 4;      // 247300

__device__ __forceinline__ bool cut_weight(int i) {
    if (i < kKerasB0) return true;                                   // W0
    if (i < kKerasBlocks || i >= kKerasWr) return false;             // b0, read-out
    return (i - kKerasBlocks) % (kHidden * kHidden + kHidden) < kHidden * kHidden;     // a hidden kernel, not its bias
}

__global__ __launch_bounds__(256) void net_range_kernel(const float* __restrict__ net, unsigned* __restrict__ out2) {
    unsigned mw = 0u, ma = 0u;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kNetVars; i += gridDim.x * blockDim.x) {
        const unsigned u = __builtin_bit_cast(unsigned, net[i]) & 0x7fffffffu;
        ma = ma > u ? ma : u;
        if (cut_weight(i)) mw = mw > u ? mw : u;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned ow = (unsigned)__shfl_xor((int)mw, off), oa = (unsigned)__shfl_xor((int)ma, off);
        mw = mw > ow ? mw : ow;
        ma = ma > oa ? ma : oa;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(out2, mw);
        atomicMax(out2 + 1, ma);
    }
}

}  // namespace

hipError_t launch_net_range(const float* net_keras, float* out2, hipStream_t st) {
    hipError_t e = launch_zero(out2, 2 * sizeof(float), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(net_range_kernel, dim3(64), dim3(256), 0, st, net_keras, reinterpret_cast<unsigned*>(out2));
    return hipGetLastError();
}

}  // namespace mvnerf
