// The Dense layers and the LayerNormalization of the ViT's transformer blocks (layers.py:72-95; encoders.py TransformerBlock) over
// token rows (M, C) fp32, row-major:
//
//   mvnerf_linear_tokens       out (M, N) = epi(x (M, K) . W^T + bias), W (N, K) in torch's Linear layout, pre-cut by mvnerf_linear_pack
//   mvnerf_layer_norm_tokens   out = ((x - mean) * rstd) * gamma + beta per row, biased variance, shifted two-pass moments
//
// The GEMM is conv3x3.hip's with one tap: fp32 grade on the fp16 matrix pipe, both operands cut into two fp16 pieces under a per-tensor
// power-of-two scale, every product block three v_mfma_f32_16x16x32_f16 (mvnerf_conv.h has the arithmetic).
//
// Tile scheme.  A workgroup (256 threads, 4 waves) owns 32 token rows and 64 output channels; wave v owns channels 16 v .. 16 v + 15 and
// both row blocks of 16: 2 accumulators of 4 registers.  The weights are the MFMA's A operand (rows = output channels), the tokens its B
// operand (columns), so a lane ends with 4 consecutive channels of one token and stores 16 bytes.  32 rows and not 64: the 591 x 768
// launches of the reference's ViT then have 19 x 12 = 228 workgroups on 256 CUs, not 120.  The last row tile is predicated: rows past M
// are zeros in LDS, never read from x and never written.
//
// K loop.  K runs in slabs of 128 (4 MFMA chunks of 32; the last slab may be shorter).  Per slab the 256 threads read 32 rows x 128
// floats (two 32-byte runs per thread, 16 consecutive threads one 512-byte run of a row), cut every element once into B0, B1 and write
// them to LDS as [piece][k group of 8][row (32 + 1 pad)][8 fp16].  Each wave streams the A fragments of its 16 channels from the packed
// stream: [channel tile][chunk][channel block][A0, A1, A0s][lane][8 fp16], one coalesced 1 KiB load per fragment.  The next slab's
// loads, tokens and weights, are issued before the products of this one.
//
// No atomics on out, no split of K, a fixed summation order: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_mfma.h"
#include "mvnerf_vit.h"

namespace mvnerf {

namespace {

constexpr int kTlThreads = 256;
constexpr int kTlRows = 32;                                   // token rows per workgroup
constexpr int kTlCout = 64;                                   // output channels per workgroup
constexpr int kTlChunk = 32;                                  // the K of one MFMA
constexpr int kTlSlabChunks = 4;                              // chunks per LDS stage
constexpr int kTlSlabGroups = 4 * kTlSlabChunks;              // k groups of 8 per stage
constexpr int kTlGroupBytes = (kTlRows + 1) * 16;             // one k group of one piece: 32 rows of 16 B and one pad slot (528)
constexpr int kTlPieceBytes = kTlSlabGroups * kTlGroupBytes;  // 8 448
constexpr int kTlLdsBytes = 2 * kTlPieceBytes;                // 16 896
constexpr int kTlStageSlots = kTlRows * kTlSlabGroups / kTlThreads;      // (row, k group) items per thread: 2
constexpr int kTlHeaderBytes = 256;                           // packed stream: [0] max |w| (float), [1] ew (int), then the fragments
constexpr int kTlFragBytes = 1024;                            // one A fragment: 64 lanes x 8 fp16
constexpr int kTlChunkBytes = 12 * kTlFragBytes;              // 4 channel blocks x 3 pieces
static_assert(kTlStageSlots * kTlThreads == kTlRows * kTlSlabGroups, "whole items per thread");
constexpr int kLnKept = 4;                                    // quads per lane the LayerNorm keeps in registers: rows of up to 1024

__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// (residual and out carry no __restrict__: they are read and written at the same index by the same lane only)
__global__ __launch_bounds__(kTlThreads, 2) void token_linear_kernel(const float* __restrict__ x, const float* __restrict__ amax_x,
                                                                     const unsigned char* __restrict__ packed, const float* __restrict__ bias,
                                                                     const float* residual, long M, int K, int N, int epi, float* out,
                                                                     unsigned* __restrict__ amax_out, int row_tiles) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kTlLdsBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const int rt = blockIdx.x % row_tiles, ct = blockIdx.x / row_tiles;      // neighbouring workgroups share a channel tile's weights
    const long row0 = (long)rt * kTlRows;
    const int ch0 = ct * kTlCout + 16 * wave + 4 * grp;                      // this lane's 4 channels; its rows are row0 + 16 tb + col

    const float max_x = *amax_x;
    const float max_w = *reinterpret_cast<const float*>(packed);
    if (!conv_amax_finite(max_x) || !conv_amax_finite(max_w)) {              // (the same in every lane of the grid)
        const float nan = __builtin_bit_cast(float, 0x7fc00000u);
        const f32x4 nan4 = {nan, nan, nan, nan};
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
            const long row = row0 + 16 * tb + col;
            if (row < M) *reinterpret_cast<f32x4*>(out + row * N + ch0) = nan4;
        }
        if (amax_out && tid == 0) atomicMax(amax_out, 0x7fc00000u);
        return;
    }
    const int ex = conv_scale_exp(max_x);
    const int ew = *reinterpret_cast<const int*>(packed + 4);

    // staging: slot s of a thread is item tid + 256 s = (row item >> 4, k group item & 15) of the slab
    f32x4 held[kTlStageSlots][2];
    auto fetch = [&](int k0, int groups) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < kTlStageSlots; ++s) {
            const int item = tid + kTlThreads * s, r = item >> 4, kg = item & 15;
            const long row = row0 + r;
            const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            held[s][0] = zero;
            held[s][1] = zero;
            if (row < M && kg < groups) {
                const f32x4* q = reinterpret_cast<const f32x4*>(x + row * K + k0 + 8 * kg);
                held[s][0] = q[0];
                held[s][1] = q[1];
            }
        }
    };
    auto commit = [&](int groups) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < kTlStageSlots; ++s) {
            const int item = tid + kTlThreads * s, r = item >> 4, kg = item & 15;
            if (kg >= groups) continue;
            const float v[8] = {held[s][0][0], held[s][0][1], held[s][0][2], held[s][0][3],
                                held[s][1][0], held[s][1][1], held[s][1][2], held[s][1][3]};
            u32x4 p0, p1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint16_t b00, b01, b10, b11;
                conv_cut_act(v[2 * k], ex, b00, b10);
                conv_cut_act(v[2 * k + 1], ex, b01, b11);
                p0[k] = (unsigned)b00 | ((unsigned)b01 << 16);
                p1[k] = (unsigned)b10 | ((unsigned)b11 << 16);
            }
            *reinterpret_cast<u32x4*>(lds + kg * kTlGroupBytes + r * 16) = p0;
            *reinterpret_cast<u32x4*>(lds + kTlPieceBytes + kg * kTlGroupBytes + r * 16) = p1;
        }
    };

    f32x4 acc[2];
    acc[0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    acc[1] = acc[0];

    const int chunks = K / kTlChunk, slabs = (chunks + kTlSlabChunks - 1) / kTlSlabChunks;
    const unsigned char* wp = packed + kTlHeaderBytes + ((size_t)ct * chunks * 12 + wave * 3) * kTlFragBytes + lane * 16;
    const unsigned char* bfrag = lds + grp * kTlGroupBytes + col * 16;
    // the A fragments of a slab: 4 chunks x 3 pieces of this wave's 16 channels, 16 bytes per lane each
    auto weights = [&](u32x4 (&wa)[kTlSlabChunks][3], int s, int nch) __attribute__((always_inline)) {
#pragma unroll
        for (int cc = 0; cc < kTlSlabChunks; ++cc)
            if (cc < nch)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    wa[cc][p] = *reinterpret_cast<const u32x4*>(wp + (size_t)(kTlSlabChunks * s + cc) * kTlChunkBytes + p * kTlFragBytes);
    };
    auto slab_chunks = [&](int s) { return chunks - kTlSlabChunks * s < kTlSlabChunks ? chunks - kTlSlabChunks * s : kTlSlabChunks; };
    u32x4 wa[kTlSlabChunks][3], wn[kTlSlabChunks][3];
    fetch(0, 4 * slab_chunks(0));
    weights(wa, 0, slab_chunks(0));
    for (int s = 0; s < slabs; ++s) {
        const int nch = slab_chunks(s);
        if (s) __syncthreads();                                  // every wave has read the previous stage
        commit(4 * nch);
        __syncthreads();
        if (s + 1 < slabs) {                                     // the next slab's tokens and weights are in flight under this one's products
            fetch((s + 1) * kTlSlabChunks * kTlChunk, 4 * slab_chunks(s + 1));
            weights(wn, s + 1, slab_chunks(s + 1));
        }
#pragma unroll
        for (int cc = 0; cc < kTlSlabChunks; ++cc)
            if (cc < nch)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb) {
                    const int off = 4 * cc * kTlGroupBytes + 16 * tb * 16;
                    const u32x4 b0 = *reinterpret_cast<const u32x4*>(bfrag + off);
                    const u32x4 b1 = *reinterpret_cast<const u32x4*>(bfrag + kTlPieceBytes + off);
                    acc[tb] = mfma16(wa[cc][2], b1, acc[tb]);            // A0s B1
                    acc[tb] = mfma16(wa[cc][1], b0, acc[tb]);            // A1 B0
                    acc[tb] = mfma16(wa[cc][0], b0, acc[tb]);            // A0 B0
                }
        if (s + 1 < slabs)
#pragma unroll
            for (int cc = 0; cc < kTlSlabChunks; ++cc)
#pragma unroll
                for (int p = 0; p < 3; ++p) wa[cc][p] = wn[cc][p];
    }

    // epilogue: un-scale, bias, gelu or residual, store; register r of acc[tb] is channel ch0 + r of row row0 + 16 tb + col
    const int undo = -(ew + ex);
    unsigned top = 0;
    f32x4 bias4 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (bias) bias4 = *reinterpret_cast<const f32x4*>(bias + ch0);
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
        const long row = row0 + 16 * tb + col;
        if (row < M) {
            f32x4 res4 = {0.0f, 0.0f, 0.0f, 0.0f};
            if (epi == kVitEpiResidual) res4 = *reinterpret_cast<const f32x4*>(residual + row * N + ch0);
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = vit_linear_epi(ldexpf(acc[tb][r], undo), bias != nullptr, bias4[r], epi, res4[r]);
                const unsigned bits = __builtin_bit_cast(unsigned, (float)v[r]) & 0x7fffffffu;
                top = bits > top ? bits : top;
            }
            *reinterpret_cast<f32x4*>(out + row * N + ch0) = v;
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

// packed stream of an (N, K) weight: fragment [channel tile ct][chunk c][channel block m][piece] of 64 lanes x 8 fp16,
// lane l, element j = W[64 ct + 16 m + (l & 15)][32 c + 8 (l >> 4) + j]
__global__ void token_linear_pack_kernel(const float* __restrict__ weight, int K, int N, unsigned char* __restrict__ packed, long total) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const float max_w = *reinterpret_cast<const float*>(packed);
    const int ew = conv_amax_finite(max_w) ? conv_scale_exp(max_w) : 0;
    if (idx == 0) *reinterpret_cast<int*>(packed + 4) = ew;
    const int j = idx & 7, l = (idx >> 3) & 63;
    long q = idx >> 9;
    const int m = q & 3;
    q >>= 2;
    const int chunks = K / kTlChunk;
    const int c = q % chunks, ct = q / chunks;
    const int k = kTlChunk * c + 8 * (l >> 4) + j, n = kTlCout * ct + 16 * m + (l & 15);
    uint16_t a0, a1, a0s;
    conv_cut_weight(weight[(size_t)n * K + k], ew, a0, a1, a0s);
    uint16_t* dst = reinterpret_cast<uint16_t*>(packed + kTlHeaderBytes) + ((((size_t)ct * chunks + c) * 4 + m) * 3) * 512 + l * 8 + j;
    dst[0] = a0;
    dst[512] = a1;
    dst[1024] = a0s;
}

// One wave per row, four rows per workgroup.  x and out may be the same array: a row is read and written by one wave, every lane its
// own quads, and the moments are complete before the first store.
__global__ __launch_bounds__(256) void layer_norm_kernel(const float* x, const float* __restrict__ gamma, const float* __restrict__ beta, long M,
                                                         int C, float eps, float* out, unsigned* __restrict__ amax_out) {
    __shared__ unsigned slot;
    if (amax_out) {
        if (threadIdx.x == 0) slot = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    const int quads = C / 4;
    unsigned top = 0;
    if (row < M) {
        const float* src = x + row * C;
        float* dst = out + row * C;
        // a row of up to 1024 channels stays in registers (4 quads per lane): one trip to memory, not three; the order is the same
        const bool kept = quads <= kLnKept * kVitLnLanes;
        f32x4 held[kLnKept];
        if (kept)
#pragma unroll
            for (int i = 0; i < kLnKept; ++i)
                if (lane + kVitLnLanes * i < quads) held[i] = *reinterpret_cast<const f32x4*>(src + 4 * (lane + kVitLnLanes * i));
        const float ref = __shfl(kept ? held[0][0] : src[0], 0);
        float mean = 0.0f, rstd = 0.0f;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {                   // the order of mvnerf_vit.h's vit_ln_lane_sum, then the butterfly
            const float centre = pass == 0 ? ref : mean;
            float s = 0.0f;
            if (kept) {
#pragma unroll
                for (int i = 0; i < kLnKept; ++i)
                    if (lane + kVitLnLanes * i < quads)
#pragma unroll
                        for (int e = 0; e < 4; ++e) s = s + (pass == 0 ? held[i][e] - centre : bn_sq_dev(held[i][e], centre));
            } else {
                for (int q = lane; q < quads; q += kVitLnLanes) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s = s + (pass == 0 ? v[e] - centre : bn_sq_dev(v[e], centre));
                }
            }
#pragma unroll
            for (int mask = 1; mask < kVitLnLanes; mask <<= 1) s = s + __shfl_xor(s, mask);
            if (pass == 0) mean = vit_ln_mean(ref, s, C);
            else rstd = vit_ln_rstd(s, C, eps);
        }
        auto apply = [&](f32x4 v, int q) __attribute__((always_inline)) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * q), b = *reinterpret_cast<const f32x4*>(beta + 4 * q);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = vit_ln_apply(v[e], mean, rstd, g[e], b[e]);
                const unsigned bits = __builtin_bit_cast(unsigned, (float)o[e]) & 0x7fffffffu;
                top = bits > top ? bits : top;
            }
            *reinterpret_cast<f32x4*>(dst + 4 * q) = o;
        };
        if (kept) {
#pragma unroll
            for (int i = 0; i < kLnKept; ++i)
                if (lane + kVitLnLanes * i < quads) apply(held[i], lane + kVitLnLanes * i);
        } else {
            for (int q = lane; q < quads; q += kVitLnLanes) apply(*reinterpret_cast<const f32x4*>(src + 4 * q), q);
        }
    }
    if (amax_out) {
        atomicMax(&slot, top);
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(amax_out, slot);
    }
}

bool linear_shape_ok(int K, int N) { return K >= kTlChunk && K % kTlChunk == 0 && N >= kTlCout && N % kTlCout == 0; }

}  // namespace

}  // namespace mvnerf

extern "C" {

size_t mvnerf_linear_packed_bytes(int K, int N) {
    using namespace mvnerf;
    if (!linear_shape_ok(K, N)) return 0;
    return (size_t)kTlHeaderBytes + (size_t)(N / 16) * (K / kTlChunk) * 3 * kTlFragBytes;
}

int mvnerf_linear_pack(const float* weight, int K, int N, void* packed, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_linear_pack";
    if (!weight || !packed) return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !weight ? "weight" : "packed");
    if (!linear_shape_ok(K, N)) return api_fail(MVNERF_E_SHAPE, "%s: K=%d N=%d (K a multiple of 32, N a multiple of 64)", who, K, N);
    if (!aligned4(weight) || !aligned16(packed))
        return api_fail(MVNERF_E_ALIGN, "%s: %s", who, !aligned4(weight) ? "weight must be 4-byte aligned" : "packed must be 16-byte aligned");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    MV_HIP(hipMemsetAsync(packed, 0, kTlHeaderBytes, st), who);
    const long total = (long)K * N;                            // one thread per weight: its three pieces
    MV_RC(mvnerf_absmax_f32(weight, total, static_cast<float*>(packed), stream));
    hipLaunchKernelGGL(token_linear_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, weight, K, N,
                       static_cast<unsigned char*>(packed), total);
    return hip_status(hipGetLastError(), who);
}

int mvnerf_linear_tokens(const float* x, const float* amax_x, const void* packed, const float* bias, const float* residual, long M, int K,
                         int N, int epi, float* out, float* amax_out, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_linear_tokens";
    if (!x || !amax_x || !packed || !out)
        return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !x ? "x" : !amax_x ? "amax_x" : !packed ? "packed" : "out");
    if (M <= 0) return api_fail(MVNERF_E_ARG, "%s: M=%ld", who, M);
    if (epi < kVitEpiBias || epi > kVitEpiResidual)
        return api_fail(MVNERF_E_SHAPE, "%s: epi=%d (0 bias, 1 bias + gelu, 2 bias + residual)", who, epi);
    if ((residual != nullptr) != (epi == kVitEpiResidual))
        return api_fail(MVNERF_E_ARG, "%s: residual goes with epi=2 (given: %s, epi=%d)", who, residual ? "yes" : "no", epi);
    if (!linear_shape_ok(K, N)) return api_fail(MVNERF_E_SHAPE, "%s: K=%d N=%d (K a multiple of 32, N a multiple of 64)", who, K, N);
    const long row_tiles = (M + kTlRows - 1) / kTlRows, blocks = row_tiles * (N / kTlCout);
    if (M > 0x7fffffffL || blocks > 0x7fffffffL)
        return api_fail(MVNERF_E_SHAPE, "%s: M=%ld N=%d is %ld tiles (rows and tiles at most 2^31 - 1 each)", who, M, N, blocks);
    if (!aligned16(x) || !aligned16(packed) || !aligned16(bias) || !aligned16(residual) || !aligned16(out))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 16-byte aligned", who,
                        !aligned16(x) ? "x" : !aligned16(packed) ? "packed" : !aligned16(bias) ? "bias" : !aligned16(residual) ? "residual" : "out");
    if (!aligned4(amax_x) || !aligned4(amax_out))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 4-byte aligned", who, !aligned4(amax_x) ? "amax_x" : "amax_out");
    hipLaunchKernelGGL(token_linear_kernel, dim3((unsigned)blocks), dim3(kTlThreads), 0, static_cast<hipStream_t>(stream), x, amax_x,
                       static_cast<const unsigned char*>(packed), bias, residual, M, K, N, epi, out, reinterpret_cast<unsigned*>(amax_out),
                       (int)row_tiles);
    return hip_status(hipGetLastError(), who);
}

int mvnerf_layer_norm_tokens(const float* x, const float* gamma, const float* beta, long M, int C, float eps, float* out, float* amax_out,
                             mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_layer_norm_tokens";
    if (!x || !gamma || !beta || !out)
        return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !x ? "x" : !gamma ? "gamma" : !beta ? "beta" : "out");
    if (M <= 0 || M > 0x7fffffffL) return api_fail(MVNERF_E_ARG, "%s: M=%ld (1 .. 2^31 - 1)", who, M);
    if (C < 4 || C % 4) return api_fail(MVNERF_E_SHAPE, "%s: C=%d (a multiple of 4)", who, C);
    if (!(eps >= 0.0f)) return api_fail(MVNERF_E_ARG, "%s: eps=%g (not negative)", who, (double)eps);
    if (!aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(out))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 16-byte aligned", who,
                        !aligned16(x) ? "x" : !aligned16(gamma) ? "gamma" : !aligned16(beta) ? "beta" : "out");
    if (!aligned4(amax_out)) return api_fail(MVNERF_E_ALIGN, "%s: amax_out must be 4-byte aligned", who);
    hipLaunchKernelGGL(layer_norm_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, gamma, beta, M, C,
                       eps, out, reinterpret_cast<unsigned*>(amax_out));
    return hip_status(hipGetLastError(), who);
}

}  // extern "C"
