// bf16 variant of the fused radiance-field kernel (BASELINE.json configs 3 and 5: bf16 weights and MFMA
// inputs, fp32 accumulate).  Same math and interfaces as field_eval.hip; what changes is the machine mapping:
//
//  * v_mfma_f32_32x32x16_bf16 runs 16x faster than the fp32 MFMA, so a wave can no longer stream its own
//    copy of the weights from L2 (that would need > 64 B/clk/CU of L1 bandwidth).  A workgroup of 8 waves
//    (8 tiles of 32 samples; one workgroup per CU, persistent over tile groups) shares them: the bf16 weight
//    stream is cut into 16 KiB segments (4 k-steps x 4 output blocks) that travel through a ring of 5 LDS buffers
//    by LDS-DMA (global_load_lds_dwordx4, no VGPR staging): while the waves run the MFMAs of segment i, the loads
//    of segments i+1..i+3 are in flight; one counted vmcnt + workgroup barrier per segment.  The waves of a
//    workgroup are in lock-step (they share the ring), so their gather / sin-cos phases leave the matrix pipe
//    idle.  Two independent 4-wave workgroups per CU, whose vector-only phases could fill the other's matrix
//    phases at twice the weight traffic, measured 10 % slower.
//  * activations stay fp32 in the accumulators (residual path, biases, read-out in fp32) and are rounded to
//    bf16 only when a register block is fed as the next MFMA's B operand (v_cvt_pk_bf16_f32); gathered
//    features are lerped in fp32, rounded once, and transposed through a wave-private bf16 LDS image.
//  * the per-(view, ray) layer-0 seed (b0 + W0_dir^T PE(dir)) is the fp32 one of dir_bias_kernel.
//  * kBits (query points, direct form): the kernel also writes one relu bit per pre-activation that the frozen trunk's backward crosses
//    (ReluBits, mvnerf_ring16.h; mvnerf_query_stash_bf16) - all that trunk_vjp_bf16_kernel (query_bf16.hip) needs of this forward.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "mvnerf_field_common.h"
#include "mvnerf_kernels.h"
#include "mvnerf_launch.h"
#include "mvnerf_math.h"
#include "mvnerf_mfma.h"
#include "mvnerf_ring16.h"

namespace mvnerf {

// ---- bf16 weight stream: 1 KiB chunks [lane][8 bf16], A operand of one (k-step of 16, 32-wide output block) ----
//   layer 0 : k-steps 0..3  = PE(cam xyz) (lower half-wave sin rows, upper cos rows) + rgb rows, 16 chunks
//             k-steps 4..19 = the 256 feature rows, 16 channels per k-step, 64 chunks
//   hidden l: k-step (kb, s): input feature 32kb + 16s + 8(j>>2) + 4h + (j&3) for element j of half h
//             (= accumulator registers 8s..8s+7 of block kb fed as B operand), 32 chunks per layer
//   read-out: 8 chunks, output rows >= 4 zero
constexpr int kW16ChunkElems = 512;
constexpr int kW16Hidden = 80, kW16Readout = 80 + 12 * 32;
constexpr int kW16Chunks = kW16Readout + 16;      // read-out: 8 chunks + 8 of padding so every segment is 16 chunks

__global__ void pack_net_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= kW16Chunks * kW16ChunkElems) return;
    const int chunk = idx / kW16ChunkElems, lane = (idx % kW16ChunkElems) / 8, jj = idx % 8;
    const int i = lane & 31, h = lane >> 5;
    float val = 0.0f;
    if (chunk < kW16Hidden) {
        const int ks = chunk / 4, nb = chunk % 4;
        int row = -1;
        if (ks < 4) {
            const int m = 8 * ks + jj;
            if (m < 30) row = (m / 10) * 20 + 2 * (m % 10) + h;
            else if (m == 30) row = 120 + h;
            else row = h ? -1 : 122;
        } else {
            row = 123 + 16 * (ks - 4) + 8 * h + jj;
        }
        if (row >= 0) val = src[kKerasW0 + row * kHidden + 32 * nb + i];
    } else if (chunk < kW16Readout) {
        const int q = chunk - kW16Hidden, layer = q / 32, r = q % 32;
        const int kbs = r / 4, nb = r % 4;
        const int f = 32 * (kbs / 2) + 16 * (kbs % 2) + 8 * (jj >> 2) + 4 * h + (jj & 3);
        const int wsrc = kKerasBlocks + (layer / 2) * kKerasBlockStride + (layer % 2) * (kHidden * kHidden + kHidden);
        val = src[wsrc + f * kHidden + 32 * nb + i];
    } else if (chunk < kW16Readout + 8) {
        const int kbs = chunk - kW16Readout;
        const int f = 32 * (kbs / 2) + 16 * (kbs % 2) + 8 * (jj >> 2) + 4 * h + (jj & 3);
        if (i < 4) val = src[kKerasWr + f * 4 + i];
    }
    dst[idx] = (__bf16)val;
}

size_t packed_net_bf16_bytes() { return (size_t)kW16Chunks * 1024 + packed_net_bf16x_bytes(); }

hipError_t launch_pack_net_bf16(const float* net_keras, void* packed16, hipStream_t st) {
    const int n = kW16Chunks * kW16ChunkElems;
    hipLaunchKernelGGL(pack_net_bf16_kernel, dim3((n + 255) / 256), dim3(256), 0, st, net_keras, static_cast<__bf16*>(packed16));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_pack_net_bf16x(net_keras, static_cast<unsigned char*>(packed16) + (size_t)kW16Chunks * 1024, st);
}

// MVNERF_BF16_KERNEL=segments pins the round-2 segment-ring kernel for the texel-table form too (A/B runs, tests of both kernels)
static bool bf16x_enabled() {
    const char* e = getenv("MVNERF_BF16_KERNEL");                        // read per launch: a test flips it inside one process
    return !(e && e[0] == 's');
}

// ---- the forward weight stream through the segment ring (mvnerf_ring16.h) -------------------------------------
// Per tile the waves consume, for every view, the layer-0 segments (PE + rgb; the feature rows unless they come from
// the texel table) and the 3 per-view blocks, then the 3 fusion blocks and the read-out.  Position p in [0, P) ->
// first chunk of the segment.
struct FwdStream {
    static __device__ __forceinline__ int start_chunk(const Ring& r, int p) {
        const int per_view = r.l0_units + kHiddenUnits;
        if (p < per_view * r.V) {
            const int q = p % per_view;
            return q < r.l0_units ? q * kSegChunks : kW16Hidden + (q - r.l0_units) * kSegChunks;
        }
        const int q = p - per_view * r.V;
        return q < kHiddenUnits ? kW16Hidden + 192 + q * kSegChunks : kW16Readout;
    }
};

// ---- texel table on the bf16 MFMA (see field_eval.hip, project_texels_kernel, for the fp32 form) --------------
// T[texel] = W0[123:379]^T features[texel] with bf16 inputs and fp32 accumulation - the same rounding the direct bf16
// kernel applies to the gathered features, 16x less matrix time than the fp32 projection (which dominates the bf16
// path on many-texel scenes).  One workgroup per 32 texels: the rows are staged in LDS as bf16 (coalesced fp32 loads,
// XOR-swizzled 16-byte chunks), wave nb runs the 16 feature k-steps of output block nb on two alternating accumulators.
// kF16: the feature maps are stored as bf16 (NHWC, 512-byte texel rows - what encoders.FeatureProducer(out_dtype=bfloat16) emits): the rows
// go to LDS as they are (16-byte chunks of 8 channels), half the HBM bytes of the pass that bounds the bf16 path on many-texel scenes.
template <bool kF16>
__global__ __launch_bounds__(512) void project_texels_bf16_kernel(const float* __restrict__ features, const f32x4* __restrict__ w16a,
                                                                  const f32x4* __restrict__ w16b, long n_texels,
                                                                  float* __restrict__ table0, float* __restrict__ table1) {
    __shared__ __attribute__((aligned(16))) unsigned char srow[32 * 512];          // 32 texels x 256 channels x bf16
    using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = wv & 3;
    const f32x4* w16 = wv < 4 ? w16a : w16b;               // waves 4..7: the second net on the same staged rows
    float* table = wv < 4 ? table0 : table1;
    const long t0 = (long)blockIdx.x * 32;
    const f32x4* fsrc = reinterpret_cast<const f32x4*>(features);
    const int nthreads = blockDim.x;
    if (kF16) {
        for (int m = 0; m < 1024 / nthreads; ++m) {
            const int idx = tid + nthreads * m;             // 16-byte chunk index inside the 32 x 32 block of bf16 rows
            const int row = idx >> 5, chunk = idx & 31;     // channels 8 chunk .. 8 chunk + 7
            long t = t0 + row;
            if (t >= n_texels) t = n_texels - 1;
            *reinterpret_cast<f32x4*>(srow + row * 512 + ((chunk ^ (row & 15)) << 4)) = fsrc[t * 32 + chunk];
        }
    } else {
        for (int m = 0; m < 2048 / nthreads; ++m) {
            const int idx = tid + nthreads * m;             // float4 index inside the 32 x 64 block
            const int row = idx >> 6, c4 = idx & 63;        // channels 4 c4 .. 4 c4 + 3
            long t = t0 + row;
            if (t >= n_texels) t = n_texels - 1;
            const f32x4 v = fsrc[t * 64 + c4];
            const int chunk = c4 >> 1;                      // 16-byte chunk of 8 channels
            *reinterpret_cast<bf16x4*>(srow + row * 512 + ((chunk ^ (row & 15)) << 4) + ((c4 & 1) << 3)) = __builtin_convertvector(v, bf16x4);
        }
    }
    __syncthreads();
    const f32x4* w = w16 + ((long)16 + nb) * 64 + lane;    // chunk (k-step 4 + ks, nb) = 4 (4 + ks) + nb
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        acc0[r] = 0.0f;
        acc1[r] = 0.0f;
    }
#pragma unroll 4
    for (int ks = 0; ks < 16; ks += 2) {
        const bf16x8 a0 = __builtin_bit_cast(bf16x8, w[(long)ks * 256]), a1 = __builtin_bit_cast(bf16x8, w[(long)(ks + 1) * 256]);
        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(srow + j * 512 + (((2 * ks + h) ^ (j & 15)) << 4));
        const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(srow + j * 512 + (((2 * ks + 2 + h) ^ (j & 15)) << 4));
        acc0 = mfma16(a0, b0, acc0);
        acc1 = mfma16(a1, b1, acc1);
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

hipError_t launch_project_texels_bf16(const float* features, const void* packed16, const void* packed16b, long n_texels, float* table,
                                      float* table1, hipStream_t stream) {
    hipLaunchKernelGGL(project_texels_bf16_kernel<false>, dim3((unsigned)((n_texels + 31) / 32)), dim3(packed16b ? 512 : 256), 0, stream,
                       features, static_cast<const f32x4*>(packed16), static_cast<const f32x4*>(packed16b), n_texels, table, table1);
    return hipGetLastError();
}

hipError_t launch_project_texels_bf16maps(const void* features_bf16, const void* packed16, const void* packed16b, long n_texels, float* table,
                                          float* table1, hipStream_t stream) {
    hipLaunchKernelGGL(project_texels_bf16_kernel<true>, dim3((unsigned)((n_texels + 31) / 32)), dim3(packed16b ? 512 : 256), 0, stream,
                       static_cast<const float*>(features_bf16), static_cast<const f32x4*>(packed16), static_cast<const f32x4*>(packed16b), n_texels,
                       table, table1);
    return hipGetLastError();
}

// one k-step (16 input rows) x 4 output blocks out of the LDS-resident segment
__device__ __forceinline__ void step16(const f32x4* wbuf, int ks_local, int lane, bf16x8 b, f32x16 (&acc)[4]) {
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const bf16x8 a = __builtin_bit_cast(bf16x8, wbuf[(ks_local * 4 + nb) * 64 + lane]);
        acc[nb] = mfma16(a, b, acc[nb]);
    }
}

__device__ __forceinline__ bf16x8 relu_to_bf16(const f32x16& v, int s) {
    // bf16(relu(x)) == relu(bf16(x)) (rounding is sign-symmetric), and on the bf16 bit pattern relu is a signed
    // 16-bit max with 0: 4 v_cvt_pk_bf16_f32 + 4 v_pk_max_i16 per 8 values instead of 16 v_max_f32 + 4 converts
    using i32x4 = __attribute__((ext_vector_type(4))) int;
    f32x8 t;
#pragma unroll
    for (int q = 0; q < 8; ++q) t[q] = v[8 * s + q];
    i32x4 r = __builtin_bit_cast(i32x4, __builtin_convertvector(t, bf16x8));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int w = r[q];
        asm("v_pk_max_i16 %0, %1, 0" : "=v"(w) : "v"(w));
        r[q] = w;
    }
    return __builtin_bit_cast(bf16x8, r);
}

// acc += W^T relu(in) for one hidden layer: 8 k-steps (input block kb = ks / 2, half ks % 2) in 8 / kKs segments
// kDrainFirst: a store was issued in front of the layer (the relu bits of `in`), so its first segment drains
template <bool kDrainFirst = false>
__device__ __forceinline__ void dense128_bf16(Ring& ring, int lane, const f32x16 (&in)[4], f32x16 (&acc)[4]) {
#pragma unroll
    for (int seg = 0; seg < 8 / kKs; ++seg) {
        segment_mfma(ring, lane, [&](int ks) {
            const int g = seg * kKs + ks;
            return relu_to_bf16(in[g >> 1], g & 1);
        }, acc);
        if (kDrainFirst && seg == 0) ring_next<true, FwdStream>(ring);
        else ring_next<false, FwdStream>(ring);
    }
}

// the lane's 64 relu bits of a pre-activation tensor (ReluBits, mvnerf_ring16.h): bit 16 nb + r = [x[nb][r] > 0]
__device__ __forceinline__ void store_relu_bits(unsigned long long* dst, const f32x16 (&x)[4]) {
    unsigned int w[2] = {0u, 0u};
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) w[nb >> 1] |= (unsigned int)(x[nb][r] > 0.0f) << (16 * (nb & 1) + r);
    *dst = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
}

constexpr int kStage16Row = 256;      // bytes per staged sample row: 128 channels x bf16

// kProj: layer 0's feature rows come from the fp32 texel table (field_eval.hip, project_texels_kernel): a 128-channel
// lerp of table rows added to the accumulators replaces the four feature segments (64 MFMAs per tile) and halves the
// gather.  All gathers run in batches of 4 iterations with their 16 loads issued up front: the 8 waves of the
// workgroup share the weight ring, hence gather at the same time, and nothing else hides that latency.
// kF16 (direct gather only): p.features holds bf16 feature maps (512-byte texel rows); the taps are widened to fp32 (exact), lerped
// in fp32 and rounded once, as with fp32 maps.
// kBits (direct gather, S = 1 query points): also writes the relu bits of the 6V + 6 pre-activations the trunk's backward needs
// (trunk_vjp_bf16_kernel, query_bf16.hip), each taken from the fp32 accumulator relu_to_bf16 is about to consume.
template <bool kMultiView, bool kProj, bool kF16, bool kBits = false>
__global__ __launch_bounds__(64 * kWgWaves, 2) void field_eval_bf16_kernel(FieldParams p, const f32x4* __restrict__ w16) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem16[];
    constexpr int kRingBytes = kRing * kSegF4 * 16;                       // 80 KiB
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned char* stage = smem16 + kRingBytes + wave * (32 * kStage16Row);   // 8 KiB per wave
    // all biases (accumulator order, fp32) live in LDS for the whole kernel: a global bias load in the middle of a
    // segment would make the in-order vmcnt wait drain the weight prefetch issued before it
    float* net = reinterpret_cast<float*>(smem16 + kRingBytes + kWgWaves * 32 * kStage16Row) - kPackB0;   // net[kPackB0 + i] -> LDS
    for (int i = tid; i < kPackBr + 8 - kPackB0; i += 64 * kWgWaves) net[kPackB0 + i] = p.net[kPackB0 + i];

    const ReluBits bits = {p.relu_bits, p.n_tiles * p.V * kBitSlots * 64};        // (kBits only)
    Ring ring;
    ring.w16 = w16;
    ring.base = reinterpret_cast<f32x4*>(smem16);
    ring.c = 0;
    ring.p = 0;
    ring.V = p.V;
    ring.l0_units = (kProj ? 16 : 80) / kSegChunks;
    ring.P = (ring.l0_units + kHiddenUnits) * p.V + kHiddenUnits + 1;
    ring.tid = tid;
    ring.wave = wave;
    ring_prime<FwdStream>(ring);

    const long n_groups = (p.n_tiles + kWgWaves - 1) / kWgWaves;
    for (long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        long tile = grp * kWgWaves + wave;
        const bool tile_ok = tile < p.n_tiles;
        if (!tile_ok) tile = p.n_tiles - 1;                               // idle waves shadow the last tile, no stores
        const LaneSample sm = lane_sample(p, tile, tile_ok, j);
        const long g = sm.g;
        const bool valid = sm.valid;
        const int b = sm.b;

        f32x16 x[4], hid[4];
        f32x16 xsum[kMultiView ? 4 : 1];

        for (int v = 0; v < p.V; ++v) {
            const int bv = b * p.V + v;
            const ViewSample vs = view_sample(p, sm, bv);
            const long vtile = kMultiView ? view_tile(p, tile, b, bv) : tile;      // (S = 1, whole tiles per scene when V > 1)
            if (valid && h == 0) store_tap_idx(p, vs);

            // ---- segment: PE(cam xyz) + rgb k-steps ----
            bias_acc<false>(p.dir_bias + 128 * vs.vray, h, x);
            float pe[32];
            rgb_inputs(p.images, vs.tl, p.W, vs.tp, h, pe);
            pe_cam_xyz(vs.cam, h, pe);
#pragma unroll
            for (int seg = 0; seg < 4 / kKs; ++seg) {
                segment_mfma(ring, lane, [&](int ks) {
                    f32x8 t;
#pragma unroll
                    for (int q = 0; q < 8; ++q) t[q] = pe[8 * (seg * kKs + ks) + q];
                    return __builtin_convertvector(t, bf16x8);
                }, x);
                ring_next<true, FwdStream>(ring);
            }

            if (kProj) {
                // ---- texel table: two passes of 64 channels (accumulator blocks nb = 2P, 2P+1 of both lane halves) ----
                // a table row is [h][nb][16]; pass P takes floats h*64 + P*32 + {0..31}: two 128-B pieces per row.
                // 16 lanes per sample row, 4 rows per load instruction, 4 taps, batches of 4 instructions per tap.
                const int l16 = lane & 15, sub = lane >> 4;
                const f32x4* tbase = reinterpret_cast<const f32x4*>(p.texel_table) + (l16 >> 3) * 16 + (l16 & 7);
#pragma unroll
                for (int P = 0; P < 2; ++P) {                       // unrolled: x[2P + nbl] must be a static register index
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 1
                    for (int it0 = 0; it0 < 8; it0 += 4) {
                        f32x4 tv[4][4];
                        float axs[4], ays[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int src = 4 * (it0 + u) + sub;
                            const int tls = __shfl(vs.tl, src);
                            axs[u] = __shfl(vs.tp.ax, src);
                            ays[u] = __shfl(vs.tp.ay, src);
                            const f32x4* f = tbase + (long)tls * 32 + P * 8;
                            tv[u][0] = f[0];
                            tv[u][1] = f[32];
                            tv[u][2] = f[(long)p.W * 32];
                            tv[u][3] = f[(long)p.W * 32 + 32];
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int src = 4 * (it0 + u) + sub;
                            *reinterpret_cast<f32x4*>(stage + src * kStage16Row + ((l16 ^ (src & 15)) << 4)) =
                                lerp_taps(tv[u][0], tv[u][1], tv[u][2], tv[u][3], axs[u], ays[u]);
                        }
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                    for (int nbl = 0; nbl < 2; ++nbl)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const f32x4 t4 = *reinterpret_cast<const f32x4*>(stage + j * kStage16Row + (((8 * h + 4 * nbl + q) ^ (j & 15)) << 4));
#pragma unroll
                            for (int c = 0; c < 4; ++c) x[2 * P + nbl][4 * q + c] += t4[c];
                        }
                }
            }
            // ---- 4 segments: the two 128-channel halves of the gathered features, 4 k-steps per segment ----
#pragma unroll 1
            for (int hf = 0; hf < (kProj ? 0 : 2); ++hf) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                const f32x4* fbase = reinterpret_cast<const f32x4*>(p.features) + hf * 32 + j;
                using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
                using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
                const u32x2* fbase16 = reinterpret_cast<const u32x2*>(p.features) + hf * 32 + j;      // 8 bytes = channels 4j .. 4j + 3 of the half row
                auto widen = [](u32x2 q) {                                  // four bf16 -> fp32, exact
                    f32x4 r;
                    r[0] = __builtin_bit_cast(float, q[0] << 16);
                    r[1] = __builtin_bit_cast(float, q[0] & 0xffff0000u);
                    r[2] = __builtin_bit_cast(float, q[1] << 16);
                    r[3] = __builtin_bit_cast(float, q[1] & 0xffff0000u);
                    return r;
                };
#pragma unroll 1
                for (int it0 = 0; it0 < 16; it0 += 4) {
                    f32x4 tv[4][4];
                    float axs[4], ays[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int src = 2 * (it0 + u) + h;
                        const int tls = __shfl(vs.tl, src);
                        axs[u] = __shfl(vs.tp.ax, src);
                        ays[u] = __shfl(vs.tp.ay, src);
                        if (kF16) {
                            const u32x2* f = fbase16 + (long)tls * 64;
                            tv[u][0] = widen(f[0]);
                            tv[u][1] = widen(f[64]);
                            tv[u][2] = widen(f[(long)p.W * 64]);
                            tv[u][3] = widen(f[(long)p.W * 64 + 64]);
                        } else {
                            const f32x4* f = fbase + (long)tls * 64;
                            tv[u][0] = f[0];
                            tv[u][1] = f[64];
                            tv[u][2] = f[(long)p.W * 64];
                            tv[u][3] = f[(long)p.W * 64 + 64];
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int src = 2 * (it0 + u) + h;
                        const f32x4 o = lerp_taps(tv[u][0], tv[u][1], tv[u][2], tv[u][3], axs[u], ays[u]);
                        // row `src`, channels 4j..4j+3 (8 bytes); 16-byte chunks XOR-swizzled by the row
                        const int off = src * kStage16Row + (((j >> 1) ^ (src & 15)) << 4) + ((j & 1) << 3);
                        *reinterpret_cast<bf16x4*>(stage + off) = __builtin_convertvector(o, bf16x4);
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int part = 0; part < 8 / kKs; ++part) {            // 8 k-steps of 16 channels per 128-channel half
                    segment_mfma(ring, lane, [&](int ks) {
                        const int off = j * kStage16Row + (((2 * (kKs * part + ks) + h) ^ (j & 15)) << 4);
                        return *reinterpret_cast<const bf16x8*>(stage + off);
                    }, x);
                    ring_next<true, FwdStream>(ring);
                }
            }

            // ---- 12 segments: the three per-view ResNet blocks ----
#pragma unroll 1
            for (int bi = 0; bi < 3; ++bi) {
                const float* bias1 = net + kPackBHidden + 256 * bi;
                bias_acc<false>(bias1, h, hid);
                if (kBits && tile_ok) store_relu_bits(bits.view(vtile, 2 * bi, lane), x);
                dense128_bf16<kBits>(ring, lane, x, hid);
                bias_acc<true>(bias1 + 128, h, x);
                if (kBits && tile_ok) store_relu_bits(bits.view(vtile, 2 * bi + 1, lane), hid);
                dense128_bf16<kBits>(ring, lane, hid, x);
            }
            if (kMultiView) {
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) xsum[nb] = (v == 0) ? x[nb] : xsum[nb] + x[nb];
            }
        }
        if (kMultiView) {
            const float nv = (float)p.V;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) x[nb] = xsum[nb] / nv;
        }

        if (p.acts_fused && valid) store_acc(p.acts_fused + 128 * g, h, x);                // complete_output: the view mean
        // ---- 12 segments: fusion blocks ----
#pragma unroll 1
        for (int bi = 3; bi < 6; ++bi) {
            const float* bias1 = net + kPackBHidden + 256 * bi;
            bias_acc<false>(bias1, h, hid);
            if (kBits && tile_ok) store_relu_bits(bits.fused(tile, 2 * (bi - 3), lane), x);
            dense128_bf16<kBits>(ring, lane, x, hid);
            bias_acc<true>(bias1 + 128, h, x);
            if (kBits && tile_ok) store_relu_bits(bits.fused(tile, 2 * (bi - 3) + 1, lane), hid);
            dense128_bf16<kBits>(ring, lane, hid, x);
            if (p.acts_fused && valid) store_acc(p.acts_fused + (long)(bi - 2) * p.total * 128 + 128 * g, h, x);
        }
        if (p.embedding && valid) store_acc(p.embedding + 128 * g, h, x);

        // ---- segment: read-out ----
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = (r < 4) ? net[kPackBr + r] : 0.0f;
        {
            const f32x4* wb = ring_cur(ring);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8 a = __builtin_bit_cast(bf16x8, wb[(kb * 2 + s) * 64 + lane]);
                    o = mfma16(a, relu_to_bf16(x[kb], s), o);
                }
        }
        if (valid && h == 0) store_readout(p.rgbs, g, o[0], o[1], o[2], o[3]);
        ring_next<true, FwdStream>(ring);                                           // stores above: drain
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                     // DMA still in flight must land before the LDS is released
}

hipError_t launch_field_eval_bf16(const FieldParams& p, const void* packed16, hipStream_t stream, bool maps_bf16) {
    if (bf16x_enabled() && field_eval_bf16x_supports(p))
        return launch_field_eval_bf16x(p, static_cast<const unsigned char*>(packed16) + (size_t)kW16Chunks * 1024, stream);
    static DeviceSetup setup;
    const int lds_bytes = kRing * kSegF4 * 16 + kWgWaves * 32 * kStage16Row + (kPackBr + 8 - kPackB0) * 4;
    int cus = 0;
    hipError_t e = device_setup(setup, {{&field_eval_bf16_kernel<false, false, false>, lds_bytes}, {&field_eval_bf16_kernel<false, true, false>, lds_bytes},
                                        {&field_eval_bf16_kernel<true, false, false>, lds_bytes}, {&field_eval_bf16_kernel<true, true, false>, lds_bytes},
                                        {&field_eval_bf16_kernel<false, false, true>, lds_bytes}, {&field_eval_bf16_kernel<true, false, true>, lds_bytes}}, &cus);
    if (e != hipSuccess) return e;
    if ((e = launch_dir_bias(p, stream)) != hipSuccess) return e;
    const long n_groups = (p.n_tiles + kWgWaves - 1) / kWgWaves;
    const long resident = (long)cus * (8 / kWgWaves);                 // persistent: as many workgroups as fit at once
    const unsigned wgs = (unsigned)(n_groups < resident ? n_groups : resident);
    const f32x4* w16 = static_cast<const f32x4*>(packed16);
#define MV16_GO(MV, PROJ, F16) hipLaunchKernelGGL((field_eval_bf16_kernel<MV, PROJ, F16>), dim3(wgs), dim3(64 * kWgWaves), lds_bytes, stream, p, w16)
    if (p.V > 1) {
        if (p.texel_table) MV16_GO(true, true, false);                     // with the table the feature maps are not read at all
        else if (maps_bf16) MV16_GO(true, false, true);
        else MV16_GO(true, false, false);
    } else {
        if (p.texel_table) MV16_GO(false, true, false);
        else if (maps_bf16) MV16_GO(false, false, true);
        else MV16_GO(false, false, false);
    }
#undef MV16_GO
    return hipGetLastError();
}

// The direct-form kernel on query points (S = 1, no texel table, fp32 maps) with the relu bits as a second output
hipError_t launch_field_eval_bf16_bits(const FieldParams& p_in, const void* packed16, void* relu_bits, hipStream_t stream) {
    FieldParams p = p_in;
    p.relu_bits = static_cast<unsigned long long*>(relu_bits);
    static DeviceSetup setup;
    const int lds_bytes = kRing * kSegF4 * 16 + kWgWaves * 32 * kStage16Row + (kPackBr + 8 - kPackB0) * 4;
    int cus = 0;
    hipError_t e = device_setup(setup, {{&field_eval_bf16_kernel<false, false, false, true>, lds_bytes},
                                        {&field_eval_bf16_kernel<true, false, false, true>, lds_bytes}}, &cus);
    if (e != hipSuccess) return e;
    if ((e = launch_dir_bias(p, stream)) != hipSuccess) return e;
    const long n_groups = (p.n_tiles + kWgWaves - 1) / kWgWaves;
    const long resident = (long)cus * (8 / kWgWaves);
    const unsigned wgs = (unsigned)(n_groups < resident ? n_groups : resident);
    const f32x4* w16 = static_cast<const f32x4*>(packed16);
    if (p.V > 1) hipLaunchKernelGGL((field_eval_bf16_kernel<true, false, false, true>), dim3(wgs), dim3(64 * kWgWaves), lds_bytes, stream, p, w16);
    else hipLaunchKernelGGL((field_eval_bf16_kernel<false, false, false, true>), dim3(wgs), dim3(64 * kWgWaves), lds_bytes, stream, p, w16);
    return hipGetLastError();
}

}  // namespace mvnerf
