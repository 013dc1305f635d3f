// The activation gate of the language fusion's backward: for out = act(y) * mul of a frozen 3x3 convolution
// (mvnerf_conv3x3_nhwc) and g = dL/dout,
//
//   mvnerf_act_gate_nhwc  d = g * mul * act'(y) over NHWC fp32, 16 bytes per lane, formed from `out` and `mul` alone (mvnerf_act_gate.h),
//                         with max |d| under the convolution's amax_out convention - the amax of the data-gradient launch that reads d.
//
// One image per blockIdx.y, so `mul` is indexed without a division by the image size.  d may be g (every lane reads its quad before it
// writes it).  No workspace, no atomics on d: bit-identical from run to run.  Stream-ordered, no host read.
#include <hip/hip_runtime.h>

#include "mvnerf_act_gate.h"
#include "mvnerf_api.h"
#include "mvnerf_mfma.h"

namespace mvnerf {

namespace {

constexpr int kActGateThreads = 256;
constexpr int kActGateMaxBlocksX = 1024;
constexpr int kActGateMaxImages = 65535;          // gridDim.y

// quads: float4 groups per image (pixels_per_image * C / 4); quads_c = C / 4
__global__ __launch_bounds__(kActGateThreads) void act_gate_kernel(const float* g, const float* __restrict__ out, const float* __restrict__ mul,
                                                                   int act, long quads, int quads_c, int C, float* d,
                                                                   unsigned* __restrict__ amax_out) {
    __shared__ unsigned slot;
    if (amax_out) {
        if (threadIdx.x == 0) slot = 0;
        __syncthreads();
    }
    const int n = blockIdx.y;
    const size_t base = (size_t)n * (size_t)quads * 4;
    const float* mul_n = mul ? mul + (size_t)n * C : nullptr;
    unsigned top = 0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const int c = (int)(q % quads_c) * 4;
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + base + q * 4);
        const f32x4 ov = *reinterpret_cast<const f32x4*>(out + base + q * 4);
        f32x4 mv = {1.0f, 1.0f, 1.0f, 1.0f};
        if (mul_n) mv = *reinterpret_cast<const f32x4*>(mul_n + c);
        f32x4 dv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dv[r] = act_gate_one(gv[r], ov[r], mv[r], act);
            const unsigned bits = __builtin_bit_cast(unsigned, (float)dv[r]) & 0x7fffffffu;
            top = bits > top ? bits : top;
        }
        *reinterpret_cast<f32x4*>(d + base + q * 4) = dv;
    }
    if (amax_out) {
        atomicMax(&slot, top);
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(amax_out, slot);
    }
}

}  // namespace

}  // namespace mvnerf

extern "C" {

int mvnerf_act_gate_nhwc(const float* g, const float* out, const float* mul, int act, int N, long pixels_per_image, int C, float* d,
                         float* amax_out, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_act_gate_nhwc";
    if (!g || !out || !d) return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !g ? "g" : !out ? "out" : "d");
    if (N <= 0 || N > kActGateMaxImages) return api_fail(MVNERF_E_ARG, "%s: N=%d (1 .. %d)", who, N, kActGateMaxImages);
    if (pixels_per_image <= 0 || pixels_per_image > 0x7fffffffL || (long)N * pixels_per_image > 0x7fffffffL)
        return api_fail(MVNERF_E_ARG, "%s: N=%d pixels_per_image=%ld (at least 1, N * pixels_per_image at most 2^31 - 1)", who, N, pixels_per_image);
    if (C < 4 || C % 4) return api_fail(MVNERF_E_SHAPE, "%s: C=%d (a multiple of 4)", who, C);
    if (act < 0 || act > 2) return api_fail(MVNERF_E_SHAPE, "%s: act=%d (0 identity, 1 relu, 2 elu)", who, act);
    if (!aligned16(g) || !aligned16(out) || !aligned16(mul) || !aligned16(d))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 16-byte aligned", who,
                        !aligned16(g) ? "g" : !aligned16(out) ? "out" : !aligned16(mul) ? "mul" : "d");
    if (!aligned4(amax_out)) return api_fail(MVNERF_E_ALIGN, "%s: amax_out must be 4-byte aligned", who);
    const long quads = pixels_per_image * (C / 4), blocks = (quads + kActGateThreads * 4 - 1) / (kActGateThreads * 4);
    hipLaunchKernelGGL(act_gate_kernel, dim3((unsigned)(blocks > kActGateMaxBlocksX ? kActGateMaxBlocksX : blocks), (unsigned)N),
                       dim3(kActGateThreads), 0, static_cast<hipStream_t>(stream), g, out, mul, act, quads, C / 4, C, d,
                       reinterpret_cast<unsigned*>(amax_out));
    return hip_status(hipGetLastError(), who);
}

}  // extern "C"
