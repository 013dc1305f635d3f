// The tail both feature producers end with, as one launch (layers.py:459-477 ConvFusion + :617-618,658-659 UpSampling2D;
// legacy_layers.py:154-191 for the image-only producer):
//
//   out (N, 2h, 2w, 256) = bilinear_x2( act([a | b]) . weight ),   a (N, h, w, Ca), b (N, h, w, Cb), weight (Ca + Cb, 256)
//
// NHWC throughout, the output in fp32 or bf16: the layout and dtype mvnerf_project_texels / the gather read.  The 1x1 convolution's
// result at the low resolution (79 MB per 240 x 320 view) lives in LDS only.
//
// Tile scheme.  A workgroup owns kTileH x kTileW = 8 x 16 low-resolution pixels and writes the 14 x 30 output pixels whose four taps
// lie inside them: with half-pixel centres output row Y blends low rows (Y - 1) >> 1 and ((Y - 1) >> 1) + 1, so the tile at low row r0
// covers output rows 2 r0 + 1 .. 2 r0 + 14 and neighbouring tiles share one low row (tile t starts at 7 t - 1; the first and the last
// tile reach over the border, where the low index clamps - that IS the border rule of the up-sampling, so no output pixel is special).
// Columns alike.  Every output pixel belongs to exactly one tile; 128 / 105 = 1.22 of the product is computed.
//
// Product.  128 pixels x K x 256 channels on the exact-fp32 MFMA (32x32x2): the pixels are the A operand's rows, the channels the B
// operand's columns, so an accumulator register is one pixel and its 32 lanes are 32 consecutive channels.  8 waves, wave v owns
// channels 32 v .. 32 v + 31 of all four 32-pixel blocks (4 accumulators).  K runs in chunks of 16: the 512 threads fetch the chunk
// (one float4 each), apply the activation once and put it into LDS (double-buffered, one barrier per chunk); the weights come straight
// from global memory (L2-resident, 2 x 128 B per load), one chunk ahead.  Inside a group of 8 k the lane half h takes k = 8 g + 4 h + e
// at step e of both operands - the sum runs over every k once in a fixed order, and the A operand is one 16-byte LDS read per 4 steps.
//
// Blend.  The accumulators go to LDS as y[pixel][256] (over the chunk buffers); a thread then takes 4 channels of a 2 x 2 output
// quad - the four outputs between the same four low pixels - blends them with the weights 9/16, 3/16, 3/16, 1/16 (rows first, then
// columns: (3/4, 1/4) or (1/4, 3/4) by parity) and stores 16 bytes (8 as bf16): a wave stores whole 1 KiB pixels.  The bf16 conversion
// (round to nearest even) is the last operation, on the value the fp32 output would hold.  No atomics, no global scratch.
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_launch.h"
#include "mvnerf_mfma.h"

namespace mvnerf {

namespace {

constexpr int kTailOut = 256;                        // output channels
constexpr int kTailThreads = 512;                    // 8 waves: one 32-channel block each
constexpr int kTileH = 8, kTileW = 16;               // low-resolution pixels of a tile (shared edges: 7 x 15 of them are new)
constexpr int kTilePix = kTileH * kTileW;            // 128 = 4 MFMA row blocks
constexpr int kChunk = 16;                           // k per LDS stage
constexpr int kLdA = kChunk + 4;                     // floats per pixel row of a stage (keeps the 16-byte reads aligned, spreads the banks)
constexpr int kStageFloats = kTilePix * kLdA;
constexpr int kTailLdsBytes = kTilePix * kTailOut * 4;      // y[128][256]; the two stages (20 KiB) lie inside it
static_assert(2 * kStageFloats * 4 <= kTailLdsBytes, "the chunk stages share the y tile's LDS");
static_assert(kTilePix * (kChunk / 4) == kTailThreads, "one float4 of a chunk per thread");

using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;

__device__ __forceinline__ float tail_act(float x, int act) {
    if (act == 1) return x > 0.0f ? x : 0.0f;
    if (act == 2) return x > 0.0f ? x : expm1f(x);
    return x;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <bool kBf16>
__global__ __launch_bounds__(kTailThreads) void fuse_upsample2x_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                       const float* __restrict__ weight, int h, int w, int Ca, int Cb, int act,
                                                                       int tiles_x, int tiles_y, void* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    int tile = blockIdx.x;
    const int tx = tile % tiles_x;
    tile /= tiles_x;
    const int ty = tile % tiles_y, n = tile / tiles_y;
    const int r0 = ty * (kTileH - 1) - 1, c0 = tx * (kTileW - 1) - 1;          // low-resolution origin of the tile (-1 at the border)
    const int K = Ca + Cb;

    // staging: thread -> (pixel of the tile, 4 channels of the chunk); its low-resolution pixel, clamped into the image
    const int s_pix = tid >> 2, s_q = tid & 3;
    const long s_row = ((long)n * h + clampi(r0 + s_pix / kTileW, h - 1)) * w + clampi(c0 + s_pix % kTileW, w - 1);
    const float* s_a = a + s_row * Ca + 4 * s_q;
    const float* s_b = b + s_row * Cb + 4 * s_q;
    auto fetch = [&](int k0) { return *reinterpret_cast<const f32x4*>(k0 < Ca ? s_a + k0 : s_b + (k0 - Ca)); };   // Ca % 16 == 0: no chunk straddles
    auto stage = [&](f32x4 v, int buf) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tail_act(v[e], act);
        *reinterpret_cast<f32x4*>(lds + buf * kStageFloats + s_pix * kLdA + 4 * s_q) = v;
    };
    // weights of a chunk for this lane: k = k0 + 8 g + 4 half + e, channel 32 wave + j
    const float* wl = weight + (long)(4 * half) * kTailOut + 32 * wave + j;
    auto fetch_w = [&](int k0, float (&bw)[8]) {
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) bw[4 * g + e] = wl[(long)(k0 + 8 * g + e) * kTailOut];
    };

    f32x16 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.0f;

    float bw[8];
    fetch_w(0, bw);
    stage(fetch(0), 0);
    __syncthreads();
    const int n_chunks = K / kChunk;
    for (int c = 0; c < n_chunks; ++c) {
        const bool more = c + 1 < n_chunks;
        f32x4 next_v = {0.0f, 0.0f, 0.0f, 0.0f};
        float next_w[8];
        if (more) {
            next_v = fetch((c + 1) * kChunk);
            fetch_w((c + 1) * kChunk, next_w);
        }
        const float* As = lds + (c & 1) * kStageFloats + j * kLdA + 4 * half;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            f32x4 av[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) av[m] = *reinterpret_cast<const f32x4*>(As + m * 32 * kLdA + 8 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[m] = mfma(av[m][e], bw[4 * g + e], acc[m]);
        }
        if (more) {
            stage(next_v, (c + 1) & 1);            // the other stage: last read in chunk c - 1, before the barrier that ended it
#pragma unroll
            for (int e = 0; e < 8; ++e) bw[e] = next_w[e];
        }
        __syncthreads();
    }

    // y[pixel][channel]: register r of block m on lane (j, half) is pixel 32 m + (r & 3) + 8 (r >> 2) + 4 half, channel 32 wave + j
    // (the barrier that ended the last chunk has retired every read of the stages this overwrites)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float val = acc[m][r];
            lds[(32 * m + (r & 3) + 8 * (r >> 2) + 4 * half) * kTailOut + 32 * wave + j] = val;
        }
    __syncthreads();

    // 2 x 2 output quads between low pixels (i, i + 1) x (q, q + 1) of the tile, 4 channels per thread
    const int H2 = 2 * h, W2 = 2 * w;
    const int c4 = 4 * (tid & 63);
    for (int quad = tid >> 6; quad < (kTileH - 1) * (kTileW - 1); quad += kTailThreads / 64) {
        const int i = quad / (kTileW - 1), q = quad % (kTileW - 1);
        const int Y0 = 2 * (r0 + i) + 1, X0 = 2 * (c0 + q) + 1;               // the quad's upper left output pixel
        if (Y0 >= H2 || X0 >= W2) continue;                                    // (wave-uniform: a quad is one wave's)
        const float* y00 = lds + (i * kTileW + q) * kTailOut + c4;
        const f32x4 v00 = *reinterpret_cast<const f32x4*>(y00), v01 = *reinterpret_cast<const f32x4*>(y00 + kTailOut),
                    v10 = *reinterpret_cast<const f32x4*>(y00 + kTileW * kTailOut),
                    v11 = *reinterpret_cast<const f32x4*>(y00 + (kTileW + 1) * kTailOut);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int Y = Y0 + dy;
            if (Y < 0 || Y >= H2) continue;
            const float wy0 = dy ? 0.25f : 0.75f, wy1 = dy ? 0.75f : 0.25f;
            const f32x4 left = wy0 * v00 + wy1 * v10, right = wy0 * v01 + wy1 * v11;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int X = X0 + dx;
                if (X < 0 || X >= W2) continue;
                const float wx0 = dx ? 0.25f : 0.75f, wx1 = dx ? 0.75f : 0.25f;
                const f32x4 o = wx0 * left + wx1 * right;
                const size_t at = (((size_t)n * H2 + Y) * W2 + X) * kTailOut + c4;
                if (kBf16)
                    *reinterpret_cast<bf16x4*>(static_cast<__bf16*>(out) + at) = __builtin_convertvector(o, bf16x4);
                else
                    *reinterpret_cast<f32x4*>(static_cast<float*>(out) + at) = o;
            }
        }
    }
}

}  // namespace

}  // namespace mvnerf

extern "C" {

int mvnerf_fuse_upsample2x(const float* a, const float* b, const float* weight, int N, int h, int w, int Ca, int Cb, int act, void* out,
                           int out_bf16, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_fuse_upsample2x";
    if (!a || !b || !weight || !out)
        return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !a ? "a" : !b ? "b" : !weight ? "weight" : "out");
    if (N <= 0 || h <= 0 || w <= 0) return api_fail(MVNERF_E_ARG, "%s: N=%d h=%d w=%d", who, N, h, w);
    if (Ca < 16 || Ca % 16) return api_fail(MVNERF_E_SHAPE, "%s: Ca=%d (a multiple of 16, at least 16)", who, Ca);
    if (Cb < 16 || Cb % 16) return api_fail(MVNERF_E_SHAPE, "%s: Cb=%d (a multiple of 16, at least 16)", who, Cb);
    if (Ca + Cb > 512) return api_fail(MVNERF_E_SHAPE, "%s: Ca+Cb=%d (at most 512)", who, Ca + Cb);
    if (act < 0 || act > 2) return api_fail(MVNERF_E_SHAPE, "%s: act=%d (0 identity, 1 relu, 2 elu)", who, act);
    const int tiles_x = w / (kTileW - 1) + 1, tiles_y = h / (kTileH - 1) + 1;
    const long tiles = (long)N * tiles_x * tiles_y;
    if (tiles > 0x7fffffffL) return api_fail(MVNERF_E_SHAPE, "%s: N=%d h=%d w=%d is %ld tiles (at most 2^31 - 1)", who, N, h, w, tiles);
    if (!aligned16(a) || !aligned16(b) || !aligned16(weight) || !aligned16(out))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 16-byte aligned", who,
                        !aligned16(a) ? "a" : !aligned16(b) ? "b" : !aligned16(weight) ? "weight" : "out");
    static DeviceSetup setup;
    MV_HIP(device_setup(setup, {{fuse_upsample2x_kernel<false>, kTailLdsBytes}, {fuse_upsample2x_kernel<true>, kTailLdsBytes}}), who);
    const auto kernel = out_bf16 ? fuse_upsample2x_kernel<true> : fuse_upsample2x_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(kTailThreads), kTailLdsBytes, static_cast<hipStream_t>(stream), a, b, weight, h, w, Ca,
                       Cb, act, tiles_x, tiles_y, out);
    return hip_status(hipGetLastError(), who);
}

}  // extern "C"
