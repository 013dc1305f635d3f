// The bf16 weight ring shared by the bf16 field kernel (field_eval_bf16.hip) and the bf16 trunk VJP (query_bf16.hip): a workgroup of
// kWgWaves waves streams 1 KiB A-operand chunks [lane][8 bf16] of v_mfma_f32_32x32x16_bf16 through a ring of LDS slots by LDS-DMA.
// What the stream holds and in which order a tile consumes it is the kernel's: a Stream type with
//   static __device__ int start_chunk(const Ring&, int p)      position p in [0, P) -> first chunk of that segment
#pragma once

#include <hip/hip_runtime.h>

#include "mvnerf_mfma.h"

namespace mvnerf {

// ---- the segment ring ----------------------------------------------------------------------------------------
// A workgroup of kWgWaves waves shares the weight stream through a ring of kRing LDS slots of kSegChunks chunks
// (kKs k-steps x 4 output blocks), filled by LDS-DMA, 2 wave-instructions (2 KiB) per wave and segment.
// The weights are the same for every tile, so positions wrap modulo P.
// The ring is LDS-DMA with 5 slots: a register-staged double buffer (two slots, no counted vmcnt) measured equal at cfg2 and
// 14 % slower at V = 3 / 480x640 (profiles/r02_ab_bf16_staged_*.log).
constexpr int kWgWaves = 8;                                    // one 512-thread workgroup per CU (see the top of field_eval_bf16.hip)
constexpr int kSegChunks = 2 * kWgWaves;                       // 16 chunks of 1 KiB
constexpr int kKs = kSegChunks / 4;                            // k-steps (of 16 rows) per segment: 4
constexpr int kRing = 5, kAhead = 3, kSegF4 = kSegChunks * 64;  // float4 per slot
constexpr int kHiddenUnits = 192 / kSegChunks;                 // segments of 3 blocks (6 Dense layers x 32 chunks)

struct Ring {
    const f32x4* w16;
    f32x4* base;        // LDS
    int c;              // ring slot of the current segment
    int p, P, V;
    int l0_units;       // forward stream: layer-0 segments per view, PE + rgb only (texel table) or PE + rgb + 256 feature rows
    int tid, wave;
};

// issue the LDS-DMA of position p + ahead into slot (c + ahead) % kRing: 2 x 16 B per thread, 1 KiB per wave-instruction
template <typename Stream>
__device__ __forceinline__ void ring_issue(const Ring& r, int ahead) {
    int pp = r.p + ahead;
    if (pp >= r.P) pp -= r.P;
    const f32x4* src = r.w16 + (long)Stream::start_chunk(r, pp) * 64 + r.tid;
    f32x4* dst = r.base + ((r.c + ahead) % kRing) * kSegF4 + 64 * r.wave;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 64 * kWgWaves),
                                     (__attribute__((address_space(3))) void*)(dst + 64 * kWgWaves), 16, 0, 0);
}

__device__ __forceinline__ const f32x4* ring_cur(const Ring& r) { return r.base + r.c * kSegF4; }

// end of a segment: the next segment's DMA (issued kAhead - 1 segments ago) must have landed for every wave.
// kDrain = false leaves the two younger segments (4 DMA instructions of this thread) in flight; segments that also
// issue ordinary loads or stores drain everything (their own waits are in-order with the DMA anyway).
template <bool kDrain, typename Stream>
__device__ __forceinline__ void ring_next(Ring& r) {
    if (kDrain) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    r.c = r.c + 1 == kRing ? 0 : r.c + 1;
    r.p = r.p + 1 == r.P ? 0 : r.p + 1;
    ring_issue<Stream>(r, kAhead);                     // slot (c + 3) % 5 was last read two segments ago; everyone is past that barrier
}

// first three segments in flight and landed, the fourth issued: the state ring_next expects
template <typename Stream>
__device__ __forceinline__ void ring_prime(Ring& r) {
    ring_issue<Stream>(r, 0);
    ring_issue<Stream>(r, 1);
    ring_issue<Stream>(r, 2);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    ring_issue<Stream>(r, kAhead);
}

__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// acc += A(segment) x B for the kKs k-steps of the LDS-resident segment
// The A operands of k-step ks+1 are requested from LDS before the MFMAs of k-step ks are issued (pinned with a
// sched_barrier: left alone the compiler keeps two A register sets and waits for an LDS round trip per MFMA pair),
// and the conversion of the next B operand runs in the shadow of those MFMAs.
// bfn(ks) -> B operand (bf16x8) of k-step ks of the segment.
template <typename BFn>
__device__ __forceinline__ void segment_mfma(Ring& ring, int lane, BFn bfn, f32x16 (&acc)[4]) {
    const f32x4* wb = ring_cur(ring) + lane;
    f32x4 a[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) a[nb] = wb[nb * 64];
    bf16x8 b = bfn(0);
#pragma unroll
    for (int ks = 0; ks < kKs; ++ks) {
        f32x4 an[4];
        if (ks < kKs - 1) {
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) an[nb] = wb[((ks + 1) * 4 + nb) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma16(__builtin_bit_cast(bf16x8, a[nb]), b, acc[nb]);
        if (ks < kKs - 1) {
            b = bfn(ks + 1);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) a[nb] = an[nb];
        }
    }
}

// ---- relu bits: what the frozen trunk's backward keeps of a forward (field_eval_bf16.hip writes, query_bf16.hip reads) ----------
// One bit per pre-activation, [fp32 accumulator > 0], for the 6 per-view slots x0,h1,x1,h2,x2,h3 of every view tile and the 6 fused
// slots mean,h4,x4,h5,x5,h6 of every tile (StashLayout's order without x3 / x6).  A (tile, slot) is 64 x 8 bytes: lane (j, h) of the
// tile's wave owns one 64-bit word, bit 16 nb + r = accumulator register r of block nb = feature 32 nb + 8 (r >> 2) + 4 h + (r & 3) of
// sample j - the registers the lane holds in both kernels, so neither shuffles.
//   words: [view tile (b V + v) tiles_per_b + k][6][64], then [tile][6][64]
constexpr int kBitSlots = 6;
struct ReluBits {
    unsigned long long* words;
    long fused_base;               // first word of the fused part: view_tiles * 6 * 64
    __device__ __forceinline__ unsigned long long* view(long view_tile, int slot, int lane) const {
        return words + (view_tile * kBitSlots + slot) * 64 + lane;
    }
    __device__ __forceinline__ unsigned long long* fused(long tile, int slot, int lane) const {
        return words + fused_base + (tile * kBitSlots + slot) * 64 + lane;
    }
};
inline size_t relu_bits_bytes(long n_tiles, int V) { return (size_t)n_tiles * (V + 1) * kBitSlots * 64 * 8; }

}  // namespace mvnerf
