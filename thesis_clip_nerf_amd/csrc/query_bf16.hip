// The frozen trunk's input gradient on the bf16 MFMA: what mvnerf_query_vjp does with twelve dense_dx launches, four
// re-layouts and an fp32 stash, as one launch that reads the cotangent rows, one relu bit per pre-activation and a bf16 weight stream.
//
//  * machine mapping of field_eval_bf16.hip: one wave per 32-point tile, 8 waves per workgroup share the weight stream through the
//    LDS-DMA ring (mvnerf_ring16.h), persistent over tile groups.  The cotangent g lives in the 4 x 16 accumulator registers per lane
//    that hold x in the forward (feature 32 nb + 8 (r >> 2) + 4 h + (r & 3) of point j), so registers 8s .. 8s+7 of block kb, rounded
//    to bf16, are the B operand of k-step (kb, s) - no lane movement anywhere.
//  * the stream: the twelve hidden kernels transposed, A[row = input feature][k = output feature], 32 chunks of 1 KiB each in the k
//    order of that B operand, in the order the walk consumes them: block 5 (W2^T, W1^T), 4, 3, then 2, 1, 0 (once per view).
//  * per block, walking backwards:  g_rh = bf16(g) W2^T;  g_hid = g_rh o bits(h);  g_x = g + (bf16(g_hid) W1^T) o bits(x)
//    with fp32 accumulation and an fp32 residual add.  The cotangents of u3, u2, u1 and the view mean are added in fp32 where those
//    tensors are produced (the order of mvnerf_query_vjp, api.hip); the mean's cotangent goes to each view as g / V (the forward's fp32
//    division mirrored; reduce_mean, layers.py:368-370), then the three per-view blocks run with that view's bits.
//  * output: g0 = dL/d(layer-0 output) in tile layout [view tile][128][32], what launch_field_dz consumes.  Layer 0 is not touched.
#include <hip/hip_runtime.h>

#include "mvnerf_kernels.h"
#include "mvnerf_launch.h"
#include "mvnerf_math.h"
#include "mvnerf_mfma.h"
#include "mvnerf_pack.h"
#include "mvnerf_ring16.h"

namespace mvnerf {

constexpr int kBwd16Layers = 12, kBwd16Chunks = kBwd16Layers * 32;        // 32 KiB per layer

// each fp32 weight rounded once, to nearest-even: the values of pack_net_bf16_kernel, transposed
__global__ void pack_bwd_streams_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= kBwd16Chunks * 512) return;
    const int chunk = idx / 512, lane = (idx % 512) / 8, jj = idx % 8;
    const int i = lane & 31, h = lane >> 5;
    const int layer = chunk / 32, r = chunk % 32, kbs = r / 4, nb = r % 4;
    const int block = 5 - layer / 2, dense = 1 - layer % 2;               // a block's second Dense first
    const int k = 32 * (kbs / 2) + 16 * (kbs % 2) + 8 * (jj >> 2) + 4 * h + (jj & 3);      // output feature of the forward
    const int wsrc = kKerasBlocks + block * kKerasBlockStride + dense * (kHidden * kHidden + kHidden);
    dst[idx] = (__bf16)src[wsrc + (32 * nb + i) * kHidden + k];
}

size_t bwd_streams_bf16_bytes() { return (size_t)kBwd16Chunks * 1024; }

hipError_t launch_pack_bwd_streams_bf16(const float* net_keras, void* bwd16, hipStream_t st) {
    const int n = kBwd16Chunks * 512;
    hipLaunchKernelGGL(pack_bwd_streams_bf16_kernel, dim3((n + 255) / 256), dim3(256), 0, st, net_keras, static_cast<__bf16*>(bwd16));
    return hipGetLastError();
}

// position p in [0, 12 + 12 V): the six fused layers, then the six per-view layers once per view
struct BwdStream {
    static __device__ __forceinline__ int start_chunk(const Ring&, int p) { return (p < 12 ? p : 12 + (p - 12) % 12) * kSegChunks; }
};

struct TrunkVjpParams {
    const float* g_acts;           // (4, total, 128) rows: cotangents of the view mean, u1, u2, u3
    ReluBits bits;                 // read only
    float* g0_tl;                  // [view tile][128][32]
    int B, V;
    long total, n_tiles;
};

// all-ones where bit k of w is set
__device__ __forceinline__ int bit_mask(unsigned int w, int k) { return (int)(w << (31 - k)) >> 31; }

__device__ __forceinline__ float masked(float v, unsigned long long w, int nb, int r) {
    const unsigned int half = nb < 2 ? (unsigned int)w : (unsigned int)(w >> 32);
    return __builtin_bit_cast(float, __builtin_bit_cast(int, v) & bit_mask(half, 16 * (nb & 1) + r));
}

// acc += A(layer) x B over the layer's 8 k-steps = 2 segments; drain_first: stores were issued since the last segment
template <typename BFn>
__device__ __forceinline__ void dense128_bwd(Ring& ring, int lane, BFn bfn, f32x16 (&acc)[4], bool drain_first) {
#pragma unroll
    for (int seg = 0; seg < 8 / kKs; ++seg) {
        segment_mfma(ring, lane, [&](int ks) { return bfn(seg * kKs + ks); }, acc);
        if (seg == 0 && drain_first) ring_next<true, BwdStream>(ring);
        else ring_next<false, BwdStream>(ring);
    }
}

// g <- dL/d(block input) from g = dL/d(block output)
__device__ __forceinline__ void block_bwd(Ring& ring, int lane, f32x16 (&g)[4], unsigned long long bits_h, unsigned long long bits_x,
                                          bool drain_first) {
    f32x16 t[4];
    zero_acc(t);
    dense128_bwd(ring, lane, [&](int gk) {
        f32x8 v;
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = g[gk >> 1][8 * (gk & 1) + q];
        return __builtin_convertvector(v, bf16x8);
    }, t, drain_first);
    bf16x8 hb[8];                                      // bf16(g_rh o bits(h)): the one rounding in the middle
#pragma unroll
    for (int gk = 0; gk < 8; ++gk) {
        f32x8 v;
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = masked(t[gk >> 1][8 * (gk & 1) + q], bits_h, gk >> 1, 8 * (gk & 1) + q);
        hb[gk] = __builtin_convertvector(v, bf16x8);
    }
    zero_acc(t);
    dense128_bwd(ring, lane, [&](int gk) { return hb[gk]; }, t, false);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) g[nb][r] = g[nb][r] + masked(t[nb][r], bits_x, nb, r);
}

// one row (128 floats) into the accumulator layout: lane (j, h) takes features 32 nb + 8 q + 4 h + {0..3}
template <bool kAdd>
__device__ __forceinline__ void load_row(const float* __restrict__ rows, long g, int h, f32x16 (&x)[4]) {
    const float* e = rows + 128 * g + 4 * h;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(e + 32 * nb + 8 * q);
#pragma unroll
            for (int c = 0; c < 4; ++c) x[nb][4 * q + c] = kAdd ? x[nb][4 * q + c] + v[c] : v[c];
        }
}

// the counterpart of store_tl (mvnerf_mfma.h): one address register, tile and block in the scalar offset, the row in the immediate
__device__ __forceinline__ void load_tl(const float* __restrict__ base, long tile, int j, int h, f32x16 (&x)[4]) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, 0xFFFFFFFF, 0x00020000);
    const int voff = (4 * h * 32 + j) * 4;
    const int tile_off = (int)((unsigned)tile * 16384u);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            x[nb][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff + ((r & 3) + 8 * (r >> 2)) * 128,
                                                                                      tile_off + nb * 4096, 0));
}

template <bool kMultiView>
__global__ __launch_bounds__(64 * kWgWaves, 2) void trunk_vjp_bf16_kernel(TrunkVjpParams p, const f32x4* __restrict__ w16) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_bwd16[];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    Ring ring;
    ring.w16 = w16;
    ring.base = reinterpret_cast<f32x4*>(smem_bwd16);
    ring.c = 0;
    ring.p = 0;
    ring.V = p.V;
    ring.l0_units = 0;
    ring.P = 12 + 12 * p.V;
    ring.tid = tid;
    ring.wave = wave;
    ring_prime<BwdStream>(ring);

    const long n_groups = (p.n_tiles + kWgWaves - 1) / kWgWaves;
    const long tiles_per_b = p.n_tiles / p.B;
    const long slab = p.total * 128;
    for (long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        long tile = grp * kWgWaves + wave;
        const bool tile_ok = tile < p.n_tiles;
        if (!tile_ok) tile = p.n_tiles - 1;                               // idle waves shadow the last tile, no stores
        long gi = tile * 32 + j;
        const bool valid = gi < p.total;                                  // the last tile's padding carries a zero cotangent
        if (!valid) gi = p.total - 1;

        f32x16 g[4];
        load_row<false>(p.g_acts + 3 * slab, gi, h, g);                   // cotangent of u3
        if (!valid) zero_acc(g);
#pragma unroll 1
        for (int bi = 5; bi >= 3; --bi) {
            const unsigned long long bh = *p.bits.fused(tile, 2 * (bi - 3) + 1, lane), bx = *p.bits.fused(tile, 2 * (bi - 3), lane);
            block_bwd(ring, lane, g, bh, bx, bi == 5);                    // (the previous tile ended with its g0 stores)
            if (valid) load_row<true>(p.g_acts + (bi - 3) * slab, gi, h, g);   // cotangents of u2, u1 and the view mean
        }
        // whole tiles per scene when V > 1: the view tile of StashLayout, (b V + v) tiles_per_b + k
        const long view0 = kMultiView ? tile + (tile / tiles_per_b) * (p.V - 1) * tiles_per_b : tile;
        const long park = view0 + (p.V - 1) * tiles_per_b;
        if (kMultiView) {
            // the mean's cotangent, g / V, is every view's starting point: it waits in the last view's g0 tile instead of in 64
            // registers (each lane re-reads what it wrote itself; idle waves leave the tile they shadow alone)
            const float nv = (float)p.V;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) g[nb] = g[nb] / nv;
            if (tile_ok) store_tl(p.g0_tl, park, j, h, g);
        }
        for (int v = 0; v < p.V; ++v) {
            const long view_tile = view0 + v * tiles_per_b;
            if (kMultiView && v > 0 && tile_ok) load_tl(p.g0_tl, park, j, h, g);
#pragma unroll 1
            for (int bi = 2; bi >= 0; --bi) {
                const unsigned long long bh = *p.bits.view(view_tile, 2 * bi + 1, lane), bx = *p.bits.view(view_tile, 2 * bi, lane);
                block_bwd(ring, lane, g, bh, bx, kMultiView && bi == 2);
            }
            if (tile_ok) store_tl(p.g0_tl, view_tile, j, h, g);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                     // DMA still in flight must land before the LDS is released
}

hipError_t launch_trunk_vjp_bf16(const void* bwd16, const void* relu_bits, const float* g_acts, int B, int V, long total, long n_tiles,
                                 float* g0_tl, hipStream_t stream) {
    static DeviceSetup setup;
    const int lds_bytes = kRing * kSegF4 * 16;
    int cus = 0;
    const hipError_t e = device_setup(setup, {{&trunk_vjp_bf16_kernel<false>, lds_bytes}, {&trunk_vjp_bf16_kernel<true>, lds_bytes}}, &cus);
    if (e != hipSuccess) return e;
    const long n_groups = (n_tiles + kWgWaves - 1) / kWgWaves;
    const unsigned wgs = (unsigned)(n_groups < cus ? n_groups : cus);     // persistent: one workgroup per CU
    TrunkVjpParams p;
    p.g_acts = g_acts;
    p.bits = {const_cast<unsigned long long*>(static_cast<const unsigned long long*>(relu_bits)), n_tiles * V * kBitSlots * 64};
    p.g0_tl = g0_tl;
    p.B = B; p.V = V; p.total = total; p.n_tiles = n_tiles;
    const f32x4* w16 = static_cast<const f32x4*>(bwd16);
    if (V > 1) hipLaunchKernelGGL(trunk_vjp_bf16_kernel<true>, dim3(wgs), dim3(64 * kWgWaves), lds_bytes, stream, p, w16);
    else hipLaunchKernelGGL(trunk_vjp_bf16_kernel<false>, dim3(wgs), dim3(64 * kWgWaves), lds_bytes, stream, p, w16);
    return hipGetLastError();
}

}  // namespace mvnerf
