// Backward of the tail both feature producers end with (feature_tail.hip), as one launch.  For g = dL/dout (N,2h,2w,256),
// X = [a | b] (N,h,w,Ca+Cb) and the weight W (Ca+Cb,256) as stored:
//
//   g_low[n,y,x,c] = sum_{Y,X'} cy(Y,y) cx(X',x) g[n,Y,X',c]         the adjoint of the x2 bilinear up-sampling, gathered
//   dX[n,y,x,k]    = act'(X[n,y,x,k]) * sum_c g_low[n,y,x,c] W[k,c]   da = dX[..., :Ca], db = dX[..., Ca:]
//
// The coefficients, the order of the adjoint's terms, act' and the tile arithmetic are mvnerf_feature_tail.h, shared with a host build.
//
// Tile scheme.  A workgroup of 512 threads owns 8 x 16 low pixels (tiles do not overlap; a ragged tile skips what lies outside the image)
// and builds their g_low tile [128][256] in LDS, rows padded by 4 floats so that the product's 16-byte reads of 32 pixels spread over the
// banks (130 KiB, one workgroup per CU).
//
// Gather.  Wave v takes low row v of the tile and walks its 16 pixels; its 64 lanes are the 64 float4 of a 1 KiB pixel, so every load of g
// and every LDS write is one whole pixel.  Rows first: v(X') = sum of the <= 4 output rows of column X', then g_low = sum of the <= 4
// columns - the order of mvnerf_feature_tail.h.  Low pixel x needs the columns 2x - 1 .. 2x + 2 and shares the last two with x + 1, so the
// walk carries them: 8 loads per low pixel instead of 16, every g element read twice (once per low row it feeds), from L2 the second time.
// Which terms exist is wave-uniform.  No atomics, no workspace.
//
// Product.  128 pixels x 256 channels of g_low against W^T on the exact-fp32 MFMA (32x32x2): the pixels are the A operand's rows (from
// LDS, one 16-byte read per 4 steps), the input channels k the B operand's columns, so an accumulator register is one pixel and its 32
// lanes are 32 consecutive k.  Column blocks of 256 k: wave v owns k = first + 256 blk + 32 v .. + 31 of all four 32-pixel blocks (4
// accumulators).  Lane (j, half) reads W[k_j][c .. c + 3] straight from global memory as 16 bytes (W is L2-resident: 512 KiB at most), 32
// channels c ahead; no transposed image is needed.  Inside a group of 8 c the lane half takes c = 8 g + 4 half + e at step e: the sum runs
// over every c once in a fixed order.  Only the requested k range is computed: [0, Ca) for da, [Ca, Ca + Cb) for db, or both.
//
// Epilogue.  Each accumulator register is one pixel x 32 consecutive k: the lanes read X there (4 bytes each, 128-byte runs; not read for
// the identity), multiply by act' and store 128-byte runs of da / db.  (The 16-byte form would need a transpose through LDS; the reads are
// 1/256 of the product's work.)
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_feature_tail.h"
#include "mvnerf_launch.h"
#include "mvnerf_mfma.h"

namespace mvnerf {

namespace {

constexpr int kFtbThreads = 512;                             // 8 waves: one low row each in the gather, one 32-k block each in the product
constexpr int kFtbLd = kFtbOut + 4;                          // floats per pixel row of the LDS tile
constexpr int kFtbLdsBytes = kFtbTilePix * kFtbLd * 4;       // 133,120
constexpr int kFtbBlockK = 32 * (kFtbThreads / 64);          // 256 input channels per column block
static_assert(kFtbThreads / 64 == kFtbTileH, "one wave per low row of the tile");
static_assert(kFtbLdsBytes <= 160 * 1024, "the g_low tile fits the CU's LDS");

__global__ __launch_bounds__(kFtbThreads) void fuse_upsample2x_bwd_kernel(const float* __restrict__ g, const float* __restrict__ a,
                                                                          const float* __restrict__ b, const float* __restrict__ weight,
                                                                          int h, int w, int Ca, int Cb, int act, int k_first, int k_end,
                                                                          float* __restrict__ da, float* __restrict__ db,
                                                                          float* __restrict__ g_low) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, half = lane >> 5;
    const FtbTile tile = ftb_tile((long)blockIdx.x, h, w);
    const int n = tile.n;

    // ---- gather: wave = low row, lane = 4 channels --------------------------------------------------------------------------------------
    {
        const int y = tile.y0 + wave, c4 = 4 * lane;
        float* row = lds + wave * kFtbTileW * kFtbLd + c4;
        const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
        if (y >= h) {                                               // (wave-uniform) a row outside the image: zeros, never stored
            for (int q = 0; q < kFtbTileW; ++q) *reinterpret_cast<f32x4*>(row + q * kFtbLd) = zero;
        } else {
            const FtbTaps ty = ftb_taps(y, h);
            const float cy0 = ty.c[0], cy1 = ty.c[1], cy2 = ty.c[2], cy3 = ty.c[3];
            const bool oy0 = ty.on[0], oy1 = ty.on[1], oy2 = ty.on[2], oy3 = ty.on[3];
            const float* g_rows = g + c4;
            const int Y0 = ty.first;
            // v(X'): the rows of output column X that feed low row y, 4 channels (every load before the first use)
            auto ftb_column = [&](int X) {
                f32x4 r0 = zero, r1 = zero, r2 = zero, r3 = zero;
                if (oy0) r0 = *reinterpret_cast<const f32x4*>(g_rows + ftb_out_offset(n, Y0, X, h, w));
                if (oy1) r1 = *reinterpret_cast<const f32x4*>(g_rows + ftb_out_offset(n, Y0 + 1, X, h, w));
                if (oy2) r2 = *reinterpret_cast<const f32x4*>(g_rows + ftb_out_offset(n, Y0 + 2, X, h, w));
                if (oy3) r3 = *reinterpret_cast<const f32x4*>(g_rows + ftb_out_offset(n, Y0 + 3, X, h, w));
                f32x4 acc = zero;
                if (oy0) acc = ftb_add(acc, cy0, r0);
                if (oy1) acc = ftb_add(acc, cy1, r1);
                if (oy2) acc = ftb_add(acc, cy2, r2);
                if (oy3) acc = ftb_add(acc, cy3, r3);
                return acc;
            };
            // the two columns the first pixel shares with its left neighbour, which another tile owns
            f32x4 v0 = zero, v1 = zero;
            if (tile.x0 > 0) {
                v0 = ftb_column(2 * tile.x0 - 1);
                v1 = ftb_column(2 * tile.x0);
            } else {
                v1 = ftb_column(0);
            }
#pragma unroll 1
            for (int q = 0; q < kFtbTileW; ++q) {
                const int x = tile.x0 + q;
                if (x >= w) {                                       // (wave-uniform)
                    *reinterpret_cast<f32x4*>(row + q * kFtbLd) = zero;
                    continue;
                }
                const FtbTaps tx = ftb_taps(x, w);
                f32x4 v2 = zero, v3 = zero;
                if (tx.on[2]) v2 = ftb_column(tx.first + 2);
                if (tx.on[3]) v3 = ftb_column(tx.first + 3);
                f32x4 acc = zero;
                if (tx.on[0]) acc = ftb_add(acc, tx.c[0], v0);
                if (tx.on[1]) acc = ftb_add(acc, tx.c[1], v1);
                if (tx.on[2]) acc = ftb_add(acc, tx.c[2], v2);
                if (tx.on[3]) acc = ftb_add(acc, tx.c[3], v3);
                *reinterpret_cast<f32x4*>(row + q * kFtbLd) = acc;
                v0 = v2;
                v1 = v3;
            }
        }
    }
    __syncthreads();

    // ---- the optional copy of the adjoint: whole 1 KiB pixels ---------------------------------------------------------------------------
    if (g_low) {
        for (int p = wave; p < kFtbTilePix; p += kFtbThreads / 64) {
            const int y = ftb_pixel_y(tile, p), x = ftb_pixel_x(tile, p);
            if (!ftb_inside(y, x, h, w)) continue;                  // (wave-uniform)
            *reinterpret_cast<f32x4*>(g_low + ftb_low_offset(n, y, x, h, w, kFtbOut) + 4 * lane) =
                *reinterpret_cast<const f32x4*>(lds + p * kFtbLd + 4 * lane);
        }
    }

    // ---- product and epilogue, one column block of 256 input channels at a time (the LDS tile is only read from here on) -----------------
    const int K = Ca + Cb;
    for (int k0 = k_first + 32 * wave; k0 < k_end; k0 += kFtbBlockK) {       // (wave-uniform)
        const int k = k0 + j;
        const bool k_on = k < k_end;                                          // Ca, Cb are multiples of 16: a block may end half way
        const float* wl = weight + (size_t)(k_on ? k : K - 1) * kFtbOut + 4 * half;
        const float* As = lds + j * kFtbLd + 4 * half;
        f32x16 acc[4];
        zero_acc(acc);
        f32x4 wv[4], wn[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) wv[s] = *reinterpret_cast<const f32x4*>(wl + 8 * s);
#pragma unroll 1
        for (int c0 = 0; c0 < kFtbOut; c0 += 32) {
            const int cn = c0 + 32 < kFtbOut ? c0 + 32 : c0;                  // (the last chunk re-reads itself: no branch around the loads)
#pragma unroll
            for (int s = 0; s < 4; ++s) wn[s] = *reinterpret_cast<const f32x4*>(wl + cn + 8 * s);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                f32x4 av[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) av[m] = *reinterpret_cast<const f32x4*>(As + m * 32 * kFtbLd + c0 + 8 * s);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int m = 0; m < 4; ++m) acc[m] = mfma(av[m][e], wv[s][e], acc[m]);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) wv[s] = wn[s];
        }

        // register r of block m: tile row 2 m + (r >> 3), column 8 ((r >> 2) & 1) + 4 half + (r & 3)   (ftb_acc_pixel)
        if (k_on) {
            const bool in_a = k < Ca;
            const int C = in_a ? Ca : Cb;
            const int x_lane = tile.x0 + 4 * half;                            // (per lane: 64 scalar offsets would not fit the SGPRs)
            const size_t first = ftb_low_offset(n, tile.y0, 0, h, w, C) + (in_a ? k : k - Ca);
            const float* xin = (in_a ? a : b) + first;
            float* dout = (in_a ? da : db) + first;
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int top = 0; top < 16; top += 8) {                       // the 8 registers of one tile row
                    const int i = ftb_acc_pixel(m, top, 0) / kFtbTileW;
                    if (tile.y0 + i >= h) continue;                           // (wave-uniform)
                    const size_t row = (size_t)i * w;
#pragma unroll
                    for (int r = top; r < top + 8; ++r) {
                        const int x = x_lane + ftb_acc_pixel(m, r, 0) % kFtbTileW;
                        if (x >= w) continue;
                        const size_t at = (row + x) * C;
                        float d = acc[m][r];
                        if (act != 0) d = ftb_act_grad(xin[at], d, act);
                        dout[at] = d;
                    }
                }
        }
    }
}

}  // namespace

}  // namespace mvnerf

extern "C" {

int mvnerf_fuse_upsample2x_bwd(const float* g, const float* a, const float* b, const float* weight, int N, int h, int w, int Ca, int Cb,
                               int act, float* da, float* db, float* g_low, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_fuse_upsample2x_bwd";
    if (!g || !weight) return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !g ? "g" : "weight");
    if (!da && !db && !g_low) return api_fail(MVNERF_E_ARG, "%s: no output wanted (da, db and g_low are all null)", who);
    if (N <= 0 || h <= 0 || w <= 0) return api_fail(MVNERF_E_ARG, "%s: N=%d h=%d w=%d", who, N, h, w);
    if (Ca < 16 || Ca % 16) return api_fail(MVNERF_E_SHAPE, "%s: Ca=%d (a multiple of 16, at least 16)", who, Ca);
    if (Cb < 16 || Cb % 16) return api_fail(MVNERF_E_SHAPE, "%s: Cb=%d (a multiple of 16, at least 16)", who, Cb);
    if (Ca + Cb > 512) return api_fail(MVNERF_E_SHAPE, "%s: Ca+Cb=%d (at most 512)", who, Ca + Cb);
    if (act < 0 || act > 2) return api_fail(MVNERF_E_SHAPE, "%s: act=%d (0 identity, 1 relu, 2 elu)", who, act);
    if (act != 0 && ((da && !a) || (db && !b)))
        return api_fail(MVNERF_E_ARG, "%s: null pointer (%s): act'=%d reads the input of every half it differentiates", who, da && !a ? "a" : "b",
                        act);
    const long tiles = ftb_tiles(N, h, w);
    if (tiles > 0x7fffffffL) return api_fail(MVNERF_E_SHAPE, "%s: N=%d h=%d w=%d is %ld tiles (at most 2^31 - 1)", who, N, h, w, tiles);
    const void* ptrs[] = {g, a, b, weight, da, db, g_low};
    const char* names[] = {"g", "a", "b", "weight", "da", "db", "g_low"};
    for (int i = 0; i < 7; ++i)
        if (!aligned16(ptrs[i])) return api_fail(MVNERF_E_ALIGN, "%s: %s must be 16-byte aligned", who, names[i]);
    static DeviceSetup setup;
    MV_HIP(device_setup(setup, {{fuse_upsample2x_bwd_kernel, kFtbLdsBytes}}), who);
    const int k_first = da ? 0 : Ca, k_end = db ? Ca + Cb : (da ? Ca : k_first);          // neither: an empty range, g_low only
    hipLaunchKernelGGL(fuse_upsample2x_bwd_kernel, dim3((unsigned)tiles), dim3(kFtbThreads), kFtbLdsBytes, static_cast<hipStream_t>(stream), g, a,
                       b, weight, h, w, Ca, Cb, act, k_first, k_end, da, db, g_low);
    return hip_status(hipGetLastError(), who);
}

}  // extern "C"
