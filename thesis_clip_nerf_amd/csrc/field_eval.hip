// Fused radiance-field evaluation for gfx950 (MI355X):
//   project -> bilinear gather -> positional encoding -> ResNet-MLP trunk -> read-out
// for 32 samples per wavefront, activations resident in the register file, weights streamed from
// L2 in MFMA operand order (mvnerf_pack.h) one 4 KiB step ahead of use, gathered features
// transposed through wave-private LDS.
//
// Reference being replaced: model_v0.py:122-144 / :157-180 (see include/mvnerf_hip.h,
// mvnerf_field_eval).  One launch evaluates B*R*S samples; a wavefront owns 32 consecutive samples
// (half a coarse ray, a quarter of a fine ray), waves are independent (no workgroup barrier).
#include <hip/hip_runtime.h>

#include "mvnerf_field_common.h"
#include "mvnerf_kernels.h"
#include "mvnerf_launch.h"
#include "mvnerf_math.h"
#include "mvnerf_pack.h"

namespace mvnerf {

// Launch shape: measured best ("What was measured on the way") is the plain one: one 32-sample tile per wave,
// 4 waves per workgroup, 2 workgroups per CU (2 waves per SIMD).  Persistent workgroups pulling tiles from an atomic ticket
// (0.739 of peak against 0.769), with raised priority for half of their waves (0.736), were slower.
constexpr int kWaves = 4;          // waves per workgroup of the single-view kernel
constexpr int kMvOcc = 2;          // waves per SIMD the multi-view kernels are compiled for: 2 spills the view sum to
                                   // scratch (132 B/lane) and is still 5 % faster than 1 (A/B, V=3: 745k -> 786k rays/s)

// acc += W^T relu(in)   (Dense 128->128 on the pre-activated input, layers.py:285-288)
__device__ __forceinline__ void dense128(WStream& ws, const f32x16 (&in)[4], f32x16 (&acc)[4]) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float raw[4] = {in[kb][4 * t], in[kb][4 * t + 1], in[kb][4 * t + 2], in[kb][4 * t + 3]};
            float b[4];
            relu4(raw, b);
            mfma_step(ws, b, acc);
        }
    }
}

// x <- x + W2^T relu(W1^T relu(x) + b1) + b2    (ResNetMLPBlock.call, layers.py:284-298)
// Training mode: `stash` (may be null) receives the two pre-activation tensors of the block in tile layout
// (slot 0: hid = input of the second Dense, slot 1: block output = input of the next layer).
template <bool kStash>
__device__ __forceinline__ void resnet_block(WStream& ws, const float* __restrict__ bias1, int h, f32x16 (&x)[4],
                                             f32x16 (&hid)[4], float* __restrict__ stash, long slot_stride, long tile,
                                             int j, bool store_out = true) {
    bias_to_acc<false>(bias1, h, hid);
    dense128(ws, x, hid);
    if (kStash) store_tl(stash, tile, j, h, hid);
    bias_to_acc<true>(bias1 + 128, h, x);
    dense128(ws, hid, x);
    if (kStash && store_out) store_tl(stash + slot_stride, tile, j, h, x);
}

// kProj: the 256 feature rows of layer 0 come from the texel table (project_texels_kernel) instead of 128 k-steps:
// layer 0 is linear in the gathered features and the bilinear gather is linear in the texels, so
// W0f^T lerp(taps) = lerp(W0f^T taps); the lerp then runs on 128 projected channels and adds into the accumulators.
template <bool kMultiView, bool kStash, bool kProj>
__global__ __launch_bounds__(kMultiView ? 256 : 64 * kWaves, kMultiView ? kMvOcc : 2) void field_eval_kernel(FieldParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];       // 16 KiB per wave

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31;
    const int h = lane >> 5;
    float* stage = lds + wave * (kTile * kStageRow);

    const long tile = (long)blockIdx.x * (blockDim.x >> 6) + wave;   // one 32-sample tile per wave
    if (tile >= p.n_tiles) return;                       // whole wave leaves; there are no barriers

    const LaneSample sm = lane_sample(p, tile, true, j);
    const long g = sm.g;
    const bool valid = sm.valid;
    const int b = sm.b;

    const float* __restrict__ net = p.net;

    f32x16 x[4], hid[4];
    f32x16 xsum[kMultiView ? 4 : 1];
    WStream ws;

    for (int v = 0; v < p.V; ++v) {
        ws_begin(ws, net, kPackTotal * 4, lane);                         // layer-0 group 0 (re-read per view)
        const int bv = b * p.V + v;
        const ViewSample vs = view_sample(p, sm, bv);
        if (valid && h == 0) {
            store_tap_idx(p, vs);
            store_pix(p, vs);
        }

        // ---- layer 0: Dense 379 -> 128 on [PE(cam xyz) | PE(cam dir) | 2*rgb-1 | features] ----
        // accumulator seed = b0 + W0_dir^T PE(cam dir) of this lane's (view, ray), from dir_bias_kernel
        bias_to_acc<false>(p.dir_bias + 128 * vs.vray, h, x);
        float pe[32];                                     // B operands of k-steps 0..31 (lower half sin, upper cos)
        pe_cam_xyz(vs.cam, h, pe);
        rgb_inputs(p.images, vs.tl, p.W, vs.tp, h, pe);
#pragma unroll
        for (int gq = 0; gq < 8; ++gq) {
            const float bb[4] = {pe[4 * gq], pe[4 * gq + 1], pe[4 * gq + 2], pe[4 * gq + 3]};
            if (kProj && gq == 7) ws.pos = kPackHidden * 4;   // the stream skips the 32 feature groups
            mfma_step(ws, bb, x);
        }
        if (kProj) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // earlier reads of `stage` are done
            const f32x4* tbase = reinterpret_cast<const f32x4*>(p.texel_table) + j;     // 32 float4 per texel row
#pragma unroll 4
            for (int it = 0; it < 16; ++it) {
                const int src = 2 * it + h;                           // sample whose 4 table rows this half-wave loads
                const int tls = __shfl(vs.tl, src);
                const float axs = __shfl(vs.tp.ax, src), ays = __shfl(vs.tp.ay, src);
                const f32x4* f = tbase + (long)tls * 32;
                const f32x4 vtl = f[0], vtr = f[32], vbl = f[(long)p.W * 32], vbr = f[(long)p.W * 32 + 32];
                *reinterpret_cast<f32x4*>(stage + stage_offset(src, j)) = lerp_taps(vtl, vtr, vbl, vbr, axs, ays);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // table rows are in accumulator order [h][nb][r]: chunk 16h + 4nb + q of row j = registers 4q..4q+3 of block nb
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 t4 = *reinterpret_cast<const f32x4*>(stage + stage_offset(j, 16 * h + 4 * nb + q));
#pragma unroll
                    for (int c = 0; c < 4; ++c) x[nb][4 * q + c] += t4[c];
                }
        }
#pragma unroll 1
        for (int hf = 0; hf < (kProj ? 0 : 2); ++hf) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // earlier reads of `stage` are done
            const f32x4* fbase = reinterpret_cast<const f32x4*>(p.features) + hf * 32 + j;
#pragma unroll 4
            for (int it = 0; it < 16; ++it) {
                const int src = 2 * it + h;                           // sample whose row this half-wave loads
                const int tls = __shfl(vs.tl, src);
                const float axs = __shfl(vs.tp.ax, src), ays = __shfl(vs.tp.ay, src);
                const f32x4* f = fbase + (long)tls * 64;
                const f32x4 vtl = f[0], vtr = f[64], vbl = f[(long)p.W * 64], vbr = f[(long)p.W * 64 + 64];
                *reinterpret_cast<f32x4*>(stage + stage_offset(src, j)) = lerp_taps(vtl, vtr, vbl, vbr, axs, ays);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // writes landed (same-wave DS order)
#pragma unroll
            for (int gg = 0; gg < 16; ++gg) {
                const f32x4 bv4 = *reinterpret_cast<const f32x4*>(stage + stage_offset(j, 2 * gg + h));
                const float bb[4] = {bv4[0], bv4[1], bv4[2], bv4[3]};
                mfma_step(ws, bb, x);
            }
        }

        const long vtile = kMultiView ? view_tile(p, tile, b, bv) : tile;              // training mode
        if (kStash) store_tl(p.stash, vtile, j, h, x);       // per-view slot 0: layer-0 output
        // ---- per-view feature blocks (layers.py:365-366); optional complete_output taps (:376-377) ----
        const long vslot = (long)p.B * p.V * p.R * p.S * 128;
        if (p.acts_view && valid) store_acc(p.acts_view + 128 * vs.vrow, h, x);
#pragma unroll 1
        for (int bi = 0; bi < 3; ++bi) {
            resnet_block<kStash>(ws, net + kPackBHidden + 256 * bi, h, x, hid,
                                 kStash ? p.stash + (1 + 2 * bi) * p.stash_stride : nullptr, p.stash_stride, vtile, j,
                                 bi < 2);                               // per-view slot 6 = x3 is not written: nothing reads it
            if (p.acts_view && valid) store_acc(p.acts_view + (bi + 1) * vslot + 128 * vs.vrow, h, x);
        }

        if (kMultiView) {                                             // reduce_mean over views (layers.py:368-370)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) xsum[nb] = (v == 0) ? x[nb] : xsum[nb] + x[nb];
        }
    }
    if (kMultiView) {
        const float nv = (float)p.V;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) x[nb] = xsum[nb] / nv;
    }

    // ---- fusion blocks (layers.py:373-374); the stream continues into hidden layer 6 ----
    if (kStash) store_tl(p.stash_fused, tile, j, h, x);                           // fused slot 0: the view mean
    if (p.acts_fused && valid) store_acc(p.acts_fused + 128 * g, h, x);           // the view mean
#pragma unroll 1
    for (int bi = 3; bi < 6; ++bi) {
        resnet_block<kStash>(ws, net + kPackBHidden + 256 * bi, h, x, hid,
                             kStash ? p.stash_fused + (1 + 2 * (bi - 3)) * p.stash_fused_stride : nullptr,
                             p.stash_fused_stride, tile, j);
        if (p.acts_fused && valid) store_acc(p.acts_fused + (bi - 2) * p.total * 128 + 128 * g, h, x);
    }

    if (p.embedding && valid) store_acc(p.embedding + 128 * g, h, x);   // optional: trunk output (layers.py:379)

    // ---- read-out: Dense 128 -> 4 on relu(x), sigmoid / softplus (layers.py:392-397) ----
    // on the vector ALU: 64 features per lane x 4 outputs = 256 FMAs, then one cross-half add - the MFMA form pads the
    // 4 outputs to a 32-row tile (64 MFMAs = 4096 matrix-pipe cycles per tile for 512 useful MACs per sample)
    f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
    {
        const f32x4* wr = reinterpret_cast<const f32x4*>(net + kPackWrPlain) + 4 * h;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const f32x4 w4 = wr[32 * nb + 8 * q + c];
                    const float a = fmaxf(x[nb][4 * q + c], 0.0f);
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = fmaf(a, w4[k], o[k]);
                }
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (o[k] + __shfl_xor(o[k], 32)) + net[kPackBr + k];
    }
    if (valid && h == 0) store_readout(p.rgbs, g, o[0], o[1], o[2], o[3]);
}

// ---- per-(view, ray) layer-0 seed (dir_seed_row, mvnerf_field_common.h): one wavefront per (b*V+v, ray) ----
__global__ __launch_bounds__(256) void dir_bias_kernel(FieldParams p) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);          // over B*V*R
    if (row >= (long)p.B * p.V * p.R) return;
    const int bv = (int)(row / p.R);
    dir_seed_row(p, bv, (int)(row - (long)bv * p.R), lane, p.net + kPackW0Dir);
}

// ---- texel table: T[b*V+v][y][x][.] = W0[123:379]^T features[b,v,y,x,:] in accumulator order [h][nb][r] ----
// One workgroup per 32 texels, one wavefront per output block nb.  The 32 feature rows (32 KiB) are staged in LDS
// with coalesced 16-byte loads (XOR-swizzled: the B operand read "lane = texel" is then conflict-free); every wave
// runs 32 steps of 4 k-steps: A = feature groups 8..39 of the packed layer-0 kernel (chunk (g, nb)), B = channels
// 8q + 4h + {0..3} of this lane's texel.  Two accumulators alternate so consecutive MFMAs do not depend on each other.
// A second net (net1 / table1, workgroups of 8 waves) shares the staged rows: coarse and fine tables from ONE read of
// the feature maps.  Split form (gridDim.y == 2, workgroups of 4 waves): workgroup (x, y) projects net y and stages the rows
// for itself - the launcher's choice while the shared form would leave compute units without a workgroup; every wave runs the
// same MFMA sequence in both forms.
// kHoist (the launcher's choice for maps of fewer blocks than compute units, where a wave has its SIMD to itself): the wave's 32 A
// chunks are requested in front of the stage and held in 128 registers; otherwise they are read four steps ahead inside the MFMA run
// (56 registers: a large map keeps four 8-wave workgroups per compute unit, whose stages and stores overlap each other's MFMAs).
template <bool kHoist>
__global__ __launch_bounds__(512) void project_texels_kernel(const float* __restrict__ features,
                                                             const float* __restrict__ net0, const float* __restrict__ net1,
                                                             long n_texels, float* __restrict__ table0,
                                                             float* __restrict__ table1) {
    __shared__ __attribute__((aligned(16))) f32x4 srow[32 * 64];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = wv & 3;
    const bool second = wv >= 4 || blockIdx.y != 0;
    const float* net = second ? net1 : net0;
    float* table = second ? table1 : table0;
    const long t0 = (long)blockIdx.x * 32;
    const f32x4* fsrc = reinterpret_cast<const f32x4*>(features);
    const int nthreads = blockDim.x;
    // the wave's 32 A chunks (32 KiB of the packed layer-0 kernel, one float4 per lane and step) do not depend on the staged rows:
    // kHoist requests all of them here, so that the MFMA run below waits for memory once and not once per group of steps
    const f32x4* w = reinterpret_cast<const f32x4*>(net) + ((long)kL0GroupFeat * 4 + nb) * 64 + lane;
    f32x4 a[kHoist ? 32 : 1];
    if (kHoist) {
#pragma unroll
        for (int q = 0; q < 32; ++q) a[q] = w[(long)q * 256];
    }
    for (int m = 0; m < 2048 / nthreads; ++m) {
        const int idx = tid + nthreads * m;                 // float4 index inside the 32 x 64 block
        const int row = idx >> 6, chunk = idx & 63;
        long t = t0 + row;
        if (t >= n_texels) t = n_texels - 1;
        srow[row * 64 + (chunk ^ (row & 15))] = fsrc[t * 64 + chunk];
    }
    __syncthreads();
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        acc0[r] = 0.0f;
        acc1[r] = 0.0f;
    }
    constexpr int kUnrollSteps = kHoist ? 16 : 4;
#pragma unroll kUnrollSteps
    for (int q = 0; q < 32; q += 2) {
        f32x4 a0, a1;
        if constexpr (kHoist) {
            a0 = a[q];
            a1 = a[q + 1];
        } else {
            a0 = w[(long)q * 256];
            a1 = w[(long)(q + 1) * 256];
        }
        const f32x4 b0 = srow[j * 64 + ((2 * q + h) ^ (j & 15))], b1 = srow[j * 64 + ((2 * q + 2 + h) ^ (j & 15))];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc0 = mfma(a0[e], b0[e], acc0);
            acc1 = mfma(a1[e], b1[e], acc1);
        }
    }
    const long t = t0 + j;
    if (t < n_texels) {
        f32x4* out = reinterpret_cast<f32x4*>(table + 128 * t + 64 * h + 16 * nb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = {acc0[4 * q] + acc1[4 * q], acc0[4 * q + 1] + acc1[4 * q + 1], acc0[4 * q + 2] + acc1[4 * q + 2],
                             acc0[4 * q + 3] + acc1[4 * q + 3]};
            out[q] = v;
        }
    }
}

hipError_t launch_project_texels(const float* features, const float* packed_net, const float* packed_net1, long n_texels,
                                 float* table, float* table1, hipStream_t stream) {
    static DeviceSetup setup;
    int cus = 0;
    hipError_t e = device_setup(setup, {}, &cus);
    if (e != hipSuccess) return e;
    const long blocks = (n_texels + 31) / 32;
    // two nets on a small map: the shared stage would occupy `blocks` compute units with two waves per SIMD queueing on one matrix
    // pipe and leave the others idle; one 4-wave workgroup per (block, net) reads the rows twice (L2) and uses twice as many units.
    // From `cus` blocks on the feature rows are the traffic and the stage stays shared.
    const bool small = blocks < cus, split = packed_net1 && small;
    const dim3 grid((unsigned)blocks, split ? 2 : 1), block(packed_net1 && !split ? 512 : 256);
    if (small) hipLaunchKernelGGL(project_texels_kernel<true>, grid, block, 0, stream, features, packed_net, packed_net1, n_texels, table, table1);
    else hipLaunchKernelGGL(project_texels_kernel<false>, grid, block, 0, stream, features, packed_net, packed_net1, n_texels, table, table1);
    return hipGetLastError();
}

// ---- weight packing -------------------------------------------------------------------------
__global__ void pack_net_kernel(const float* __restrict__ src, float* __restrict__ dst) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= kPackTotal) return;
    float val = 0.0f;
    // position inside a 1 KiB chunk: [lane][e]
    const int e = idx % 4, lane = (idx % kChunkFloats) / 4, i = lane & 31, h = lane >> 5;
    if (idx < kPackHidden) {                                          // layer-0 kernel
        const int G = idx / kGroupFloats, nb = (idx % kGroupFloats) / kChunkFloats;
        int row = -1;
        if (G < kL0GroupFeat) {
            const int ks = 4 * G + e;
            if (ks < 30) row = (ks / 10) * 20 + 2 * (ks % 10) + h;       // sin | cos of PE(xyz)
            else if (ks == 30) row = 120 + h;                            // r | g
            else row = h ? -1 : 122;                                     // b | 0
        } else {
            const int q = G - kL0GroupFeat;
            row = 123 + 128 * (q / 16) + 8 * (q % 16) + 4 * h + e;
        }
        if (row >= 0) val = src[kKerasW0 + row * kHidden + 32 * nb + i];
    } else if (idx < kPackWr) {                                       // 12 hidden Dense kernels
        const int q = idx - kPackHidden;
        const int layer = q / kHiddenWFloats, r = q % kHiddenWFloats;
        const int wsrc = kKerasBlocks + (layer / 2) * kKerasBlockStride + (layer % 2) * (kHidden * kHidden + kHidden);
        const int grp = r / kGroupFloats, nb = (r % kGroupFloats) / kChunkFloats;
        const int kb = grp / 4, t = grp % 4;
        val = src[wsrc + (32 * kb + 8 * t + 4 * h + e) * kHidden + 32 * nb + i];
    } else if (idx < kPackB0) {                                       // read-out kernel, rows >= 4 zero
        const int chunk = (idx - kPackWr) / kChunkFloats;
        const int kb = chunk / 4, t = chunk % 4;
        if (i < 4) val = src[kKerasWr + (32 * kb + 8 * t + 4 * h + e) * 4 + i];
    } else if (idx < kPackBr) {                                       // biases, [h][nb][r] per layer
        const int q = idx - kPackB0;
        const int layer = q / 128, qq = q % 128;                      // 0 = layer 0, 1..12 = hidden
        const int feat = 32 * ((qq % 64) / 16) + acc_row(qq % 16, qq / 64);
        if (layer == 0) val = src[kKerasB0 + feat];
        else {
            const int l = layer - 1;
            val = src[kKerasBlocks + (l / 2) * kKerasBlockStride + (l % 2) * (kHidden * kHidden + kHidden) +
                      kHidden * kHidden + feat];
        }
    } else if (idx < kPackBr + 4) {
        val = src[kKerasBr + (idx - kPackBr)];
    } else if (idx >= kPackW0Dir && idx < kPackB0Plain) {             // plain W0 rows 60..119 (PE of cam dir)
        val = src[kKerasW0 + 60 * kHidden + (idx - kPackW0Dir)];
    } else if (idx >= kPackWrPlain) {
        val = src[kKerasWr + (idx - kPackWrPlain)];
    } else if (idx >= kPackB0Plain) {
        val = src[kKerasB0 + (idx - kPackB0Plain)];
    }
    dst[idx] = val;
}

hipError_t launch_pack_net(const float* net_keras, float* packed, hipStream_t stream) {
    const int threads = 256;
    hipLaunchKernelGGL(pack_net_kernel, dim3((kPackTotal + threads - 1) / threads), dim3(threads), 0, stream,
                       net_keras, packed);
    return hipGetLastError();
}

hipError_t launch_dir_bias(const FieldParams& p, hipStream_t stream) {
    const long rows = (long)p.B * p.V * p.R;
    hipLaunchKernelGGL(dir_bias_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_field_eval(const FieldParams& p, hipStream_t stream) {
    static DeviceSetup setup;
    const int lds_sv = kWaves * kTile * kStageRow * 4, lds_mv = 4 * kTile * kStageRow * 4;
    hipError_t e = device_setup(setup, {{&field_eval_kernel<false, false, false>, lds_sv}, {&field_eval_kernel<false, false, true>, lds_sv},
                                        {&field_eval_kernel<false, true, false>, lds_sv}, {&field_eval_kernel<false, true, true>, lds_sv},
                                        {&field_eval_kernel<true, false, false>, lds_mv}, {&field_eval_kernel<true, false, true>, lds_mv},
                                        {&field_eval_kernel<true, true, false>, lds_mv}, {&field_eval_kernel<true, true, true>, lds_mv}});
    if (e != hipSuccess) return e;
    if ((e = launch_dir_bias(p, stream)) != hipSuccess) return e;
    const int waves = p.V > 1 ? 4 : kWaves;
    const unsigned wgs = (unsigned)((p.n_tiles + waves - 1) / waves);
    const size_t lds_bytes = (size_t)waves * kTile * kStageRow * 4;
    if (p.V > 1) {
        if (p.stash) {
            if (((long)p.R * p.S) % 32 != 0) return hipErrorInvalidValue;     // tiles must not straddle scenes
            if (p.texel_table) hipLaunchKernelGGL((field_eval_kernel<true, true, true>), dim3(wgs), dim3(256), lds_bytes, stream, p);
            else hipLaunchKernelGGL((field_eval_kernel<true, true, false>), dim3(wgs), dim3(256), lds_bytes, stream, p);
        } else if (p.texel_table) {
            hipLaunchKernelGGL((field_eval_kernel<true, false, true>), dim3(wgs), dim3(256), lds_bytes, stream, p);
        } else {
            hipLaunchKernelGGL((field_eval_kernel<true, false, false>), dim3(wgs), dim3(256), lds_bytes, stream, p);
        }
    } else if (p.stash) {
        if (p.texel_table) hipLaunchKernelGGL((field_eval_kernel<false, true, true>), dim3(wgs), dim3(64 * kWaves), lds_bytes, stream, p);
        else hipLaunchKernelGGL((field_eval_kernel<false, true, false>), dim3(wgs), dim3(64 * kWaves), lds_bytes, stream, p);
    } else if (p.texel_table) {
        hipLaunchKernelGGL((field_eval_kernel<false, false, true>), dim3(wgs), dim3(64 * kWaves), lds_bytes, stream, p);
    } else {
        hipLaunchKernelGGL((field_eval_kernel<false, false, false>), dim3(wgs), dim3(64 * kWaves), lds_bytes, stream, p);
    }
    return hipGetLastError();
}

}  // namespace mvnerf
