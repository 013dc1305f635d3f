// Batch-statistics normalisation behind the 3x3 convolution (layers.py:7-34 `Block`: BatchNormalization(training=True) after each
// convolution, then the skip and the relu), as two small passes over what mvnerf_conv3x3_nhwc_ex left behind:
//
//   mvnerf_bn_finalize    the per-tile (mean, M2) partials of one convolution -> mean[c], rstd[c] = 1 / sqrt(var + eps), biased variance.
//                         The tiles are combined with Chan's pairwise update in double, in a fixed order: 16 runs of consecutive tiles
//                         per channel, then the 16 runs in order.  Pixel counts follow from (h, w) and the tile size.
//   mvnerf_bn_apply_nhwc  out = act(((y - mean[c]) * rstd[c]) * gamma[c] + beta[c] (+ skip)) over NHWC fp32, 16 bytes per lane, with max |out|
//                         under the convolution's amax_out convention.  Subtract first: y * s + (beta - mean * s) cancels when |mean| >> sigma.
//
// The arithmetic is mvnerf_conv.h (also built for the host by tests/cpu_bn).  Stream-ordered, no host read, no float atomics.
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_conv.h"
#include "mvnerf_mfma.h"

namespace mvnerf {

namespace {

// block = 64 channels of one channel tile x 16 runs; stats is [channel tile][image][tile row][tile column][mean | M2][64]
__global__ __launch_bounds__(kBnCout* kBnRuns) void bn_finalize_kernel(const float* __restrict__ stats, int N, int h, int w, int Cout, double eps,
                                                                      float* __restrict__ mean, float* __restrict__ rstd) {
    __shared__ BnMoments part[kBnRuns][kBnCout];
    const int c = threadIdx.x & (kBnCout - 1), run = threadIdx.x / kBnCout, ct = blockIdx.x;
    const size_t tiles = (size_t)N * ((h + kBnTile - 1) / kBnTile) * ((w + kBnTile - 1) / kBnTile);
    BnMoments acc = bn_combine_run(stats + ct * tiles * 2 * kBnCout + c, run, N, h, w);
    part[run][c] = acc;
    __syncthreads();
    if (run == 0) {
        for (int r = 1; r < kBnRuns; ++r) acc = bn_chan_combine(acc, part[r][c]);
        mean[ct * kBnCout + c] = (float)acc.mean;
        rstd[ct * kBnCout + c] = bn_rstd(acc, eps);
    }
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float* y, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, const float* skip, long quads,
                                                       int C, int act, float* out, unsigned* __restrict__ amax_out) {
    __shared__ unsigned slot;
    if (amax_out) {
        if (threadIdx.x == 0) slot = 0;
        __syncthreads();
    }
    unsigned top = 0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
        const int c = (int)((q * 4) % C);
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + q * 4);
        const f32x4 m = *reinterpret_cast<const f32x4*>(mean + c), s = *reinterpret_cast<const f32x4*>(rstd + c);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c), b = *reinterpret_cast<const f32x4*>(beta + c);
        f32x4 k = {0.0f, 0.0f, 0.0f, 0.0f};
        if (skip) k = *reinterpret_cast<const f32x4*>(skip + q * 4);
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o[r] = bn_apply_one(v[r], m[r], s[r], g[r], b[r], skip != nullptr, k[r], act);
            const unsigned bits = __builtin_bit_cast(unsigned, (float)o[r]) & 0x7fffffffu;
            top = bits > top ? bits : top;
        }
        *reinterpret_cast<f32x4*>(out + q * 4) = o;
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

int mvnerf_bn_finalize(const float* stats, int N, int h, int w, int Cout, double eps, float* mean, float* rstd, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_bn_finalize";
    if (!stats || !mean || !rstd) return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !stats ? "stats" : !mean ? "mean" : "rstd");
    if (N <= 0 || h <= 0 || w <= 0) return api_fail(MVNERF_E_ARG, "%s: N=%d h=%d w=%d", who, N, h, w);
    if (Cout < kBnCout || Cout % kBnCout) return api_fail(MVNERF_E_SHAPE, "%s: Cout=%d (a multiple of 64, at least 64)", who, Cout);
    if (!(eps >= 0.0)) return api_fail(MVNERF_E_ARG, "%s: eps=%g (not negative)", who, eps);
    const long tiles = (long)N * ((h + kBnTile - 1) / kBnTile) * ((w + kBnTile - 1) / kBnTile);
    if ((long)N * h * w > 0x7fffffffL || tiles * (Cout / kBnCout) > 0x7fffffffL)
        return api_fail(MVNERF_E_SHAPE, "%s: N=%d h=%d w=%d Cout=%d (pixels and tiles at most 2^31 - 1 each)", who, N, h, w, Cout);
    if (!aligned16(stats) || !aligned4(mean) || !aligned4(rstd))
        return api_fail(MVNERF_E_ALIGN, "%s: %s", who, !aligned16(stats) ? "stats must be 16-byte aligned" : "mean and rstd must be 4-byte aligned");
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)(Cout / kBnCout)), dim3(kBnCout * kBnRuns), 0, static_cast<hipStream_t>(stream), stats, N,
                       h, w, Cout, eps, mean, rstd);
    return hip_status(hipGetLastError(), who);
}

int mvnerf_bn_apply_nhwc(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* skip, long pixels,
                         int C, int act, float* out, float* amax_out, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_bn_apply_nhwc";
    if (!y || !mean || !rstd || !gamma || !beta || !out)
        return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who,
                        !y ? "y" : !mean ? "mean" : !rstd ? "rstd" : !gamma ? "gamma" : !beta ? "beta" : "out");
    if (pixels <= 0 || pixels > 0x7fffffffL) return api_fail(MVNERF_E_ARG, "%s: pixels=%ld (1 .. 2^31 - 1)", who, pixels);
    if (C < 4 || C % 4) return api_fail(MVNERF_E_SHAPE, "%s: C=%d (a multiple of 4)", who, C);
    if (act < 0 || act > 1) return api_fail(MVNERF_E_SHAPE, "%s: act=%d (0 identity, 1 relu)", who, act);
    if (!aligned16(y) || !aligned16(mean) || !aligned16(rstd) || !aligned16(gamma) || !aligned16(beta) || !aligned16(skip) || !aligned16(out))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 16-byte aligned", who,
                        !aligned16(y) ? "y" : !aligned16(mean) ? "mean" : !aligned16(rstd) ? "rstd" : !aligned16(gamma) ? "gamma" :
                        !aligned16(beta) ? "beta" : !aligned16(skip) ? "skip" : "out");
    if (!aligned4(amax_out)) return api_fail(MVNERF_E_ALIGN, "%s: amax_out must be 4-byte aligned", who);
    const long quads = pixels * (C / 4), blocks = (quads + 256 * 4 - 1) / (256 * 4);
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), y, mean, rstd,
                       gamma, beta, skip, quads, C, act, out, reinterpret_cast<unsigned*>(amax_out));
    return hip_status(hipGetLastError(), who);
}

}  // extern "C"
