// Bias-free, stride-1, zero-padded 3x3 convolution over NHWC fp32 maps as one launch: the seven 3x3 convolutions of CombineCLIPVisualV4
// (layers.py:414-456, 593-660; encoders.py DoubleConv / Up) with the front end and epilogue the fusion U-Net needs:
//
//   y[n, i, j, co] = mul[n, co] * act( sum_{dy, dx} sum_c X[n, i + dy - 1, j + dx - 1, c] * W[dy, dx, c, co] ),   X = [a | b] along c
//
// An implicit GEMM on the fp16 matrix pipe at fp32 grade: both operands are cut into two fp16 pieces under a per-tensor power-of-two
// scale and every product block is three v_mfma_f32_16x16x32_f16 (mvnerf_conv.h has the arithmetic).
//
// Tile scheme.  A workgroup (256 threads, 4 waves) owns 16 x 16 output pixels of one image and 64 output channels; wave v owns rows
// 4 v .. 4 v + 3 of the tile (4 pixel blocks of 16) and all 64 channels (4 channel blocks of 16): 16 accumulators of 4 registers.  The
// weights are the MFMA's A operand (rows = output channels), the pixels its B operand (columns), so a lane ends with 4 consecutive
// channels of one pixel per accumulator and stores 16 bytes.
//
// K loop.  K = 9 (Ca + Cb) runs as chunks of 32 input channels, the nine taps inside a chunk.  Per chunk the 256 threads read the
// 18 x 18 halo of the tile (zeros outside the image: predication, no padded copy; [a | b] from its two sources), cut every element ONCE
// into B0, B1 and write them to LDS as [piece][k group of 8][pixel (336)][8 fp16]: the B fragment of a tap is then a 16-byte read at a
// shifted pixel index - 16 consecutive pixels are 16 consecutive 16-byte slots and the k groups lie a multiple of 256 bytes apart, so every
// lane group of a ds_read_b128 covers the 64 banks once.  The weights stream from global memory as the pre-cut pieces in the order
// the loop consumes them: 12 KiB per (channel tile, chunk, tap) = [channel block][A0, A1, A0s][lane][8 fp16], one coalesced 1 KiB
// load per fragment (the four waves of a workgroup read the same 12 KiB).
//
// Scales.  ea, eb from the device words amax_a, amax_b, ew from the packed stream's header: all inside the kernel, no host read.  The
// accumulators are in units of 2^-(ew + ea) while `a` runs; at the a -> b boundary they are multiplied by 2^(eb - ea) (ldexpf, exact), the
// epilogue multiplies by 2^-(ew + e_last).  A non-finite amax (or weight maximum) fills the tile with NaN instead.
//
// No atomics on out, no workspace, a fixed summation order: two runs give the same bits.
//
// mvnerf_conv3x3_nhwc_ex (the convolutions of VisualFeatures, layers.py:7-34, 206-212) adds, as compile-time variants that
// leave the plain instantiation's code as it was: a bias in front of the activation, an activation of the source elements as the halo
// is read (before the cut; the padding stays zero), and per-workgroup (mean, M2) partials of what the tile writes, for batchnorm.hip.
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_conv.h"
#include "mvnerf_launch.h"
#include "mvnerf_mfma.h"

namespace mvnerf {

namespace {

constexpr int kCvThreads = 256;
constexpr int kCvTile = 16;                                   // output pixels per tile side
constexpr int kCvHalo = kCvTile + 2;                          // 18
constexpr int kCvHaloPix = kCvHalo * kCvHalo;                 // 324
constexpr int kCvPixPad = 336;                                // pixels per k group in LDS: 336 * 16 B = 21 * 256 B
constexpr int kCvCout = 64;                                   // output channels per workgroup
constexpr int kCvChunk = 32;                                  // input channels per LDS stage = the K of one MFMA
constexpr int kCvGroupBytes = kCvPixPad * 16;                 // one k group of one piece
constexpr int kCvPieceBytes = 4 * kCvGroupBytes;
constexpr int kCvLdsBytes = 2 * kCvPieceBytes;                // 43 008
constexpr int kCvStageItems = kCvHaloPix * 4;                 // (pixel, k group) pairs of a stage: 1296
constexpr int kCvStageSlots = (kCvStageItems + kCvThreads - 1) / kCvThreads;      // 6 per thread
constexpr int kCvHeaderBytes = 256;                           // packed stream: [0] max |w| (float), [1] ew (int), then the fragments
constexpr int kCvFragBytes = 1024;                            // one A fragment: 64 lanes x 8 fp16
constexpr int kCvTapBytes = 12 * kCvFragBytes;                // 4 channel blocks x 3 pieces
static_assert(kCvGroupBytes % 256 == 0, "the k groups of a B fragment must fall on the same banks");
static_assert(kCvHaloPix <= kCvPixPad, "halo fits its LDS row");

// (the plain instantiation's epilogue; the variants of mvnerf_conv3x3_nhwc_ex use mvnerf_conv.h's conv_act_f, the same function for host and device)
__device__ __forceinline__ float conv_act(float x, int act) {
    if (act == 1) return x > 0.0f ? x : 0.0f;
    if (act == 2) return x > 0.0f ? x : expm1f(x);
    return x;
}

__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// What mvnerf_conv3x3_nhwc_ex adds to a launch: the trailing argument of the kernels behind it.  The plain instantiation has no such
// argument (an empty pack), so its code and its argument block are what they were.
struct ConvEx {
    const float* bias;          // (Cout) or null
    float* stats;               // [workgroup][mean | M2][64] or null
};
__device__ __forceinline__ ConvEx conv_ex() { return ConvEx{nullptr, nullptr}; }
__device__ __forceinline__ ConvEx conv_ex(ConvEx ex) { return ex; }

// kActIn: the activation of the source elements as the halo is read (0 identity, 1 relu, 2 elu); Ex: nothing, or one ConvEx.
template <int kActIn, class... Ex>
__global__ __launch_bounds__(kCvThreads, 2) void conv3x3_kernel(const float* __restrict__ a, const float* __restrict__ b, int Ca, int Cb,
                                                             const float* __restrict__ amax_a, const float* __restrict__ amax_b,
                                                             const unsigned char* __restrict__ packed, int N, int h, int w, int Cout, int act,
                                                             const float* __restrict__ mul, float* __restrict__ out,
                                                             unsigned* __restrict__ amax_out, int tiles_x, int tiles_y, Ex... extra) {
    constexpr bool kEx = sizeof...(Ex) != 0;
    [[maybe_unused]] const ConvEx ex = conv_ex(extra...);
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, grp = lane >> 4;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    bid /= tiles_y;
    const int n = bid % N, ct = bid / N;
    const int y0 = ty * kCvTile, x0 = tx * kCvTile;

    // the epilogue's pixels and channels of this lane: pixel block nb is tile row 4 wave + nb, column `col`; channels 16 m + 4 grp .. + 3
    const int px = x0 + col;
    const int ch0 = ct * kCvCout + 4 * grp;

    const float max_a = *amax_a, max_b = Cb ? *amax_b : 0.0f;
    const float max_w = *reinterpret_cast<const float*>(packed);
    if (!conv_amax_finite(max_a) || !conv_amax_finite(max_b) || !conv_amax_finite(max_w)) {       // (the same in every lane of the grid)
        const float nan = __builtin_bit_cast(float, 0x7fc00000u);
        const f32x4 nan4 = {nan, nan, nan, nan};
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int py = y0 + 4 * wave + nb;
            if (py < h && px < w)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    *reinterpret_cast<f32x4*>(out + (((size_t)n * h + py) * w + px) * Cout + ch0 + 16 * m) = nan4;
        }
        if (amax_out && tid == 0) atomicMax(amax_out, 0x7fc00000u);
        if constexpr (kEx) {
            if (ex.stats && tid < 2 * kCvCout) ex.stats[(size_t)blockIdx.x * 2 * kCvCout + tid] = nan;
        }
        return;
    }
    const int ea = conv_scale_exp(max_a), eb = conv_scale_exp(max_b);
    const int ew = *reinterpret_cast<const int*>(packed + 4);

    // staging: slot s of a thread is item tid + 256 s = (halo pixel, k group); its image pixel, or -1 outside the image
    int src_pix[kCvStageSlots];
#pragma unroll
    for (int s = 0; s < kCvStageSlots; ++s) {
        const int item = tid + kCvThreads * s, hp = item >> 2;
        const int iy = y0 - 1 + hp / kCvHalo, ix = x0 - 1 + hp % kCvHalo;
        src_pix[s] = (item < kCvStageItems && iy >= 0 && iy < h && ix >= 0 && ix < w) ? (n * h + iy) * w + ix : -1;
    }
    auto stage = [&](const float* __restrict__ src, int C, int c0, int e) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < kCvStageSlots; ++s) {
            const int item = tid + kCvThreads * s;
            if (item >= kCvStageItems) break;
            const int hp = item >> 2, g = item & 3;
            f32x4 lo = {0.0f, 0.0f, 0.0f, 0.0f}, hi = lo;
            if (src_pix[s] >= 0) {
                const f32x4* q = reinterpret_cast<const f32x4*>(src + (size_t)src_pix[s] * C + c0 + 8 * g);
                lo = q[0];
                hi = q[1];
            }
            float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            if constexpr (kActIn != 0) {                            // act_in(0) == 0: the taps outside the image stay zero
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = conv_act_f(v[k], kActIn);
            }
            u32x4 p0, p1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint16_t b00, b01, b10, b11;
                conv_cut_act(v[2 * k], e, b00, b10);
                conv_cut_act(v[2 * k + 1], e, b01, b11);
                p0[k] = (unsigned)b00 | ((unsigned)b01 << 16);
                p1[k] = (unsigned)b10 | ((unsigned)b11 << 16);
            }
            *reinterpret_cast<u32x4*>(lds + g * kCvGroupBytes + hp * 16) = p0;
            *reinterpret_cast<u32x4*>(lds + kCvPieceBytes + g * kCvGroupBytes + hp * 16) = p1;
        }
    };

    f32x4 acc[4][4];                     // [channel block m][pixel block nb]
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[m][nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int chunks_a = Ca / kCvChunk, chunks = (Ca + Cb) / kCvChunk;
    const unsigned char* wp = packed + kCvHeaderBytes + (size_t)ct * chunks * 9 * kCvTapBytes + lane * 16;
    const unsigned char* bfrag = lds + grp * kCvGroupBytes + ((4 * wave) * kCvHalo + col) * 16;
    for (int c = 0; c < chunks; ++c) {
        if (c) __syncthreads();                                  // every wave has read the previous stage
        if (c < chunks_a) {
            stage(a, Ca, c * kCvChunk, ea);
        } else {
            if (c == chunks_a && ea != eb) {                      // from here on the accumulators count in units of 2^-(ew + eb)
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[m][nb][r] = ldexpf(acc[m][nb][r], eb - ea);
            }
            stage(b, Cb, (c - chunks_a) * kCvChunk, eb);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3, dx = t % 3;
            u32x4 wa[4][3];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int p = 0; p < 3; ++p) wa[m][p] = *reinterpret_cast<const u32x4*>(wp + (m * 3 + p) * kCvFragBytes);
            wp += kCvTapBytes;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const int off = ((nb + dy) * kCvHalo + dx) * 16;
                const u32x4 b0 = *reinterpret_cast<const u32x4*>(bfrag + off);
                const u32x4 b1 = *reinterpret_cast<const u32x4*>(bfrag + kCvPieceBytes + off);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    acc[m][nb] = mfma16(wa[m][2], b1, acc[m][nb]);            // A0s B1
                    acc[m][nb] = mfma16(wa[m][1], b0, acc[m][nb]);            // A1 B0
                    acc[m][nb] = mfma16(wa[m][0], b0, acc[m][nb]);            // A0 B0
                }
            }
        }
    }

    // epilogue: un-scale, activation, mul, store; register r of acc[m][nb] is channel ch0 + 16 m + r of pixel (4 wave + nb, col)
    const int undo = -(ew + (Cb ? eb : ea));
    unsigned top = 0;
    if constexpr (kEx) {
        // the same epilogue with the bias in front of the activation; the written values stay in the accumulators for the statistics
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            f32x4 bias4 = {0.0f, 0.0f, 0.0f, 0.0f}, mul4 = {1.0f, 1.0f, 1.0f, 1.0f};
            if (ex.bias) bias4 = *reinterpret_cast<const f32x4*>(ex.bias + ch0 + 16 * m);
            if (mul) mul4 = *reinterpret_cast<const f32x4*>(mul + (size_t)n * Cout + ch0 + 16 * m);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const int py = y0 + 4 * wave + nb;
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sum = ldexpf(acc[m][nb][r], undo);
                    v[r] = ex.bias ? conv_bias_act(sum, bias4[r], act) : conv_act_f(sum, act);
                    if (mul) v[r] = v[r] * mul4[r];
                }
                acc[m][nb] = v;
                if (py >= h || px >= w) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned bits = __builtin_bit_cast(unsigned, (float)v[r]) & 0x7fffffffu;
                    top = bits > top ? bits : top;
                }
                *reinterpret_cast<f32x4*>(out + (((size_t)n * h + py) * w + px) * Cout + ch0 + 16 * m) = v;
            }
        }
        if (ex.stats) {                                          // (the same in every thread)
            // Per channel over the tile's real pixels: mean = ref + sum(y - ref) / k with ref the tile's first pixel, then M2 about that
            // mean (mvnerf_conv.h).  A channel's 256 pixels lie in 4 registers (nb) x 16 lanes (col) x 4 waves: registers, then an
            // xor butterfly over the 16 lanes, then the four waves in order through LDS.  Every order is fixed.
            float* red = reinterpret_cast<float*>(lds);          // [0, 64) ref, then mean; [64, 320) one row of 64 per wave
            const int chl = 4 * grp;                             // this lane's channels of the tile: 16 m + chl + r
            const int count = conv_tile_pixels(h, w, ty, tx, kCvTile);
            bool real[4];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) real[nb] = y0 + 4 * wave + nb < h && px < w;
            __syncthreads();                                     // the last stage has been read
            if (wave == 0 && col == 0)
#pragma unroll
                for (int m = 0; m < 4; ++m) *reinterpret_cast<f32x4*>(red + 16 * m + chl) = acc[m][0];
            __syncthreads();
            f32x4 centre[4];                                     // ref in the first pass, the mean in the second
#pragma unroll
            for (int m = 0; m < 4; ++m) centre[m] = *reinterpret_cast<const f32x4*>(red + 16 * m + chl);
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                f32x4 part[4];
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float s = 0.0f;
#pragma unroll
                        for (int nb = 0; nb < 4; ++nb) {
                            const float t = pass == 0 ? acc[m][nb][r] - centre[m][r] : bn_sq_dev(acc[m][nb][r], centre[m][r]);
                            s = s + (real[nb] ? t : 0.0f);
                        }
#pragma unroll
                        for (int mask = 1; mask < 16; mask <<= 1) s = s + __shfl_xor(s, mask);
                        part[m][r] = s;
                    }
                if (pass) __syncthreads();                       // the means have been read
                if (col == 0)
#pragma unroll
                    for (int m = 0; m < 4; ++m) *reinterpret_cast<f32x4*>(red + 64 + 64 * wave + 16 * m + chl) = part[m];
                __syncthreads();
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float* q = red + 64 + 16 * m + chl;
                    const f32x4 total = ((*reinterpret_cast<const f32x4*>(q) + *reinterpret_cast<const f32x4*>(q + 64)) +
                                         *reinterpret_cast<const f32x4*>(q + 128)) + *reinterpret_cast<const f32x4*>(q + 192);
                    if (pass == 0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) centre[m][r] = bn_tile_mean(centre[m][r], total[r], count);
                    }
                    if (wave == 0 && col == 0)                   // this workgroup's own slots: plain stores, no atomics
                        *reinterpret_cast<f32x4*>(ex.stats + ((size_t)blockIdx.x * 2 + pass) * kCvCout + 16 * m + chl) = pass == 0 ? centre[m] : total;
                }
            }
        }
    } else {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int py = y0 + 4 * wave + nb;
            if (py >= h || px >= w) continue;
            float* o = out + (((size_t)n * h + py) * w + px) * Cout + ch0;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = conv_act(ldexpf(acc[m][nb][r], undo), act);
                if (mul) v = v * *reinterpret_cast<const f32x4*>(mul + (size_t)n * Cout + ch0 + 16 * m);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned bits = __builtin_bit_cast(unsigned, (float)v[r]) & 0x7fffffffu;
                    top = bits > top ? bits : top;
                }
                *reinterpret_cast<f32x4*>(o + 16 * m) = v;
            }
        }
    }
    if (amax_out) {                                              // (the same in every thread)
        unsigned* slot = reinterpret_cast<unsigned*>(lds);
        __syncthreads();                                         // the last stage has been read
        if (tid == 0) *slot = 0;
        __syncthreads();
        atomicMax(slot, top);
        __syncthreads();
        if (tid == 0) atomicMax(amax_out, *slot);
    }
}

// packed stream of a (3, 3, cin, cout) kernel: fragment [channel tile ct][chunk c][tap t][channel block m][piece] of 64 lanes x 8 fp16,
// lane l, element j = W[t / 3][t % 3][32 c + 8 (l >> 4) + j][64 ct + 16 m + (l & 15)]
__global__ void conv3x3_pack_kernel(const float* __restrict__ w_hwio, int cin, int cout, unsigned char* __restrict__ packed, long total) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const float max_w = *reinterpret_cast<const float*>(packed);
    const int ew = conv_amax_finite(max_w) ? conv_scale_exp(max_w) : 0;
    if (idx == 0) *reinterpret_cast<int*>(packed + 4) = ew;
    const int j = idx & 7, l = (idx >> 3) & 63;
    long q = idx >> 9;
    const int m = q & 3;
    q >>= 2;
    const int t = q % 9;
    q /= 9;
    const int chunks = cin / kCvChunk;
    const int c = q % chunks, ct = q / chunks;
    const int ci = kCvChunk * c + 8 * (l >> 4) + j, co = kCvCout * ct + 16 * m + (l & 15);
    uint16_t a0, a1, a0s;
    conv_cut_weight(w_hwio[((size_t)t * cin + ci) * cout + co], ew, a0, a1, a0s);
    uint16_t* dst = reinterpret_cast<uint16_t*>(packed + kCvHeaderBytes) + ((((size_t)ct * chunks + c) * 9 + t) * 12 + m * 3) * 512 + l * 8 + j;
    dst[0] = a0;
    dst[512] = a1;
    dst[1024] = a0s;
}

// max |x| as the bit pattern of a non-negative float under an unsigned max: a NaN (pattern above infinity's) stays a NaN
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ amax) {
    __shared__ unsigned slot;
    if (threadIdx.x == 0) slot = 0;
    __syncthreads();
    unsigned top = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const unsigned bits = __builtin_bit_cast(unsigned, x[i]) & 0x7fffffffu;
        top = bits > top ? bits : top;
    }
    atomicMax(&slot, top);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(amax, slot);
}

int launch_absmax(const float* x, long n, float* amax, hipStream_t st, const char* who) {
    MV_HIP(hipMemsetAsync(amax, 0, sizeof(float), st), who);
    const long blocks = (n + 256 * 16 - 1) / (256 * 16);
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks))), dim3(256), 0, st, x, n,
                       reinterpret_cast<unsigned*>(amax));
    return hip_status(hipGetLastError(), who);
}

bool conv_channels_ok(int cin, int cout) { return cin >= kCvChunk && cin % kCvChunk == 0 && cout >= kCvCout && cout % kCvCout == 0; }

// mvnerf_conv3x3_nhwc (bias, act_in, stats = null, 0, null: the plain instantiation) and mvnerf_conv3x3_nhwc_ex: the checks, then one launch
int conv3x3_call(const char* who, const float* a, int Ca, const float* amax_a, const float* b, int Cb, const float* amax_b, const void* packed,
                 int N, int h, int w, int Cout, int act, const float* mul, float* out, float* amax_out, const float* bias, int act_in,
                 float* stats, mvnerf_stream_t stream) {
    if (!a || !amax_a || !packed || !out)
        return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !a ? "a" : !amax_a ? "amax_a" : !packed ? "packed" : "out");
    if ((b != nullptr) != (Cb != 0) || (b != nullptr) != (amax_b != nullptr))
        return api_fail(MVNERF_E_ARG, "%s: b, Cb=%d and amax_b go together (all given, or NULL, 0, NULL)", who, Cb);
    if (N <= 0 || h <= 0 || w <= 0) return api_fail(MVNERF_E_ARG, "%s: N=%d h=%d w=%d", who, N, h, w);
    if (Ca < kCvChunk || Ca % kCvChunk) return api_fail(MVNERF_E_SHAPE, "%s: Ca=%d (a multiple of 32, at least 32)", who, Ca);
    if (Cb < 0 || Cb % kCvChunk) return api_fail(MVNERF_E_SHAPE, "%s: Cb=%d (a multiple of 32, or 0 without b)", who, Cb);
    if (Cout < kCvCout || Cout % kCvCout) return api_fail(MVNERF_E_SHAPE, "%s: Cout=%d (a multiple of 64, at least 64)", who, Cout);
    if (act < 0 || act > 2) return api_fail(MVNERF_E_SHAPE, "%s: act=%d (0 identity, 1 relu, 2 elu)", who, act);
    if (act_in < 0 || act_in > 2) return api_fail(MVNERF_E_SHAPE, "%s: act_in=%d (0 identity, 1 relu, 2 elu)", who, act_in);
    const int tiles_x = (w + kCvTile - 1) / kCvTile, tiles_y = (h + kCvTile - 1) / kCvTile;
    const long pixels = (long)N * h * w, blocks = (long)N * tiles_x * tiles_y * (Cout / kCvCout);
    if (pixels > 0x7fffffffL || blocks > 0x7fffffffL)
        return api_fail(MVNERF_E_SHAPE, "%s: N=%d h=%d w=%d Cout=%d is %ld pixels in %ld tiles (each at most 2^31 - 1)", who, N, h, w, Cout, pixels,
                        blocks);
    if (!aligned16(a) || !aligned16(b) || !aligned16(packed) || !aligned16(mul) || !aligned16(out))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 16-byte aligned", who,
                        !aligned16(a) ? "a" : !aligned16(b) ? "b" : !aligned16(packed) ? "packed" : !aligned16(mul) ? "mul" : "out");
    if (!aligned16(bias) || !aligned16(stats))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 16-byte aligned", who, !aligned16(bias) ? "bias" : "stats");
    if (!aligned4(amax_a) || !aligned4(amax_b) || !aligned4(amax_out))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 4-byte aligned", who, !aligned4(amax_a) ? "amax_a" : !aligned4(amax_b) ? "amax_b" : "amax_out");
    static DeviceSetup setup;
    MV_HIP(device_setup(setup, {{conv3x3_kernel<0>, kCvLdsBytes}, {conv3x3_kernel<0, ConvEx>, kCvLdsBytes},
                                {conv3x3_kernel<1, ConvEx>, kCvLdsBytes}, {conv3x3_kernel<2, ConvEx>, kCvLdsBytes}}), who);
    const dim3 grid((unsigned)blocks), block(kCvThreads);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned char* pk = static_cast<const unsigned char*>(packed);
    unsigned* top = reinterpret_cast<unsigned*>(amax_out);
    if (!bias && !act_in && !stats) {
        hipLaunchKernelGGL(conv3x3_kernel<0>, grid, block, kCvLdsBytes, st, a, b, Ca, Cb, amax_a, amax_b, pk, N, h, w, Cout, act, mul, out, top,
                           tiles_x, tiles_y);
    } else {
        const ConvEx ex{bias, stats};
        auto* kernel = act_in == 0 ? conv3x3_kernel<0, ConvEx> : act_in == 1 ? conv3x3_kernel<1, ConvEx> : conv3x3_kernel<2, ConvEx>;
        hipLaunchKernelGGL(kernel, grid, block, kCvLdsBytes, st, a, b, Ca, Cb, amax_a, amax_b, pk, N, h, w, Cout, act, mul, out, top, tiles_x,
                           tiles_y, ex);
    }
    return hip_status(hipGetLastError(), who);
}

}  // namespace

}  // namespace mvnerf

extern "C" {

size_t mvnerf_conv3x3_packed_bytes(int cin, int cout) {
    using namespace mvnerf;
    if (!conv_channels_ok(cin, cout)) return 0;
    return (size_t)kCvHeaderBytes + (size_t)(cout / 16) * (cin / kCvChunk) * 9 * 3 * kCvFragBytes;
}

int mvnerf_conv3x3_pack(const float* w_hwio, int cin, int cout, void* packed, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_conv3x3_pack";
    if (!w_hwio || !packed) return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !w_hwio ? "w_hwio" : "packed");
    if (!conv_channels_ok(cin, cout))
        return api_fail(MVNERF_E_SHAPE, "%s: cin=%d cout=%d (cin a multiple of 32, cout a multiple of 64)", who, cin, cout);
    if (!aligned4(w_hwio) || !aligned16(packed))
        return api_fail(MVNERF_E_ALIGN, "%s: %s", who, !aligned4(w_hwio) ? "w_hwio must be 4-byte aligned" : "packed must be 16-byte aligned");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    MV_HIP(hipMemsetAsync(packed, 0, kCvHeaderBytes, st), who);
    MV_RC(launch_absmax(w_hwio, 9L * cin * cout, static_cast<float*>(packed), st, who));
    const long total = 9L * cin * cout;                        // one thread per weight: its three pieces
    hipLaunchKernelGGL(conv3x3_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w_hwio, cin, cout,
                       static_cast<unsigned char*>(packed), total);
    return hip_status(hipGetLastError(), who);
}

int mvnerf_absmax_f32(const float* x, long n, float* amax, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_absmax_f32";
    if (!x || !amax) return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !x ? "x" : "amax");
    if (n <= 0) return api_fail(MVNERF_E_ARG, "%s: n=%ld", who, n);
    if (!aligned4(x) || !aligned4(amax)) return api_fail(MVNERF_E_ALIGN, "%s: %s must be 4-byte aligned", who, !aligned4(x) ? "x" : "amax");
    return launch_absmax(x, n, amax, static_cast<hipStream_t>(stream), who);
}

int mvnerf_conv3x3_nhwc(const float* a, int Ca, const float* amax_a, const float* b, int Cb, const float* amax_b, const void* packed, int N,
                        int h, int w, int Cout, int act, const float* mul, float* out, float* amax_out, mvnerf_stream_t stream) {
    return mvnerf::conv3x3_call("mvnerf_conv3x3_nhwc", a, Ca, amax_a, b, Cb, amax_b, packed, N, h, w, Cout, act, mul, out, amax_out, nullptr, 0,
                                nullptr, stream);
}

size_t mvnerf_conv3x3_stats_bytes(int N, int h, int w, int Cout) {
    using namespace mvnerf;
    if (N <= 0 || h <= 0 || w <= 0 || Cout < kCvCout || Cout % kCvCout) return 0;
    const size_t tiles = (size_t)N * ((h + kCvTile - 1) / kCvTile) * ((w + kCvTile - 1) / kCvTile);
    return tiles * (Cout / kCvCout) * 2 * kCvCout * sizeof(float);
}

int mvnerf_conv3x3_nhwc_ex(const float* a, int Ca, const float* amax_a, const float* b, int Cb, const float* amax_b, const void* packed, int N,
                           int h, int w, int Cout, int act, const float* mul, float* out, float* amax_out, const float* bias, int act_in,
                           float* stats, mvnerf_stream_t stream) {
    return mvnerf::conv3x3_call("mvnerf_conv3x3_nhwc_ex", a, Ca, amax_a, b, Cb, amax_b, packed, N, h, w, Cout, act, mul, out, amax_out, bias,
                                act_in, stats, stream);
}

}  // extern "C"
