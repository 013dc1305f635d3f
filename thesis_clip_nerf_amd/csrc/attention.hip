// Self-attention of the ViT's transformer blocks (layers.py:72-95, tf.keras MultiHeadAttention on (x, x); encoders.py KerasMHA) as one
// launch over the QKV GEMM's output as it lies:
//
//   qkv (B, n, 3, heads, d) fp32  ->  out (B, n, heads d) = softmax_j(q_i . k_j * scale) v_j   per image and head
//
// fp32 throughout, on the exact fp32 MFMA v_mfma_f32_16x16x4_f32: no 16-bit rounding of q, k, v or of the probabilities.
//
// A workgroup (256 threads, 4 waves) serves one (image, head) and up to 64 queries, one block of 16 queries per wave.  K and V of the
// head are staged once in LDS as [key][d + 4] floats (the pad spreads 16 keys over the 64 banks); keys past n are zeros.
//
// Layout.  Keys are the MFMA's rows and queries its columns: S^T block kb = K[16 kb ..][:] Q^T has, on lane (col, grp), the logits of
// query `col` against the keys 16 kb + 4 grp + r, r = 0..3.  All n <= 256 keys are 16 such blocks = 64 registers, so the softmax is the
// plain one: the row maximum (registers, then the 4 lane groups by xor 16, 32), w = expf(s - max) with the accurate expf, the row sum the
// same way.  Keys past n get the logit -inf, hence the weight exactly 0.  The weights never leave their registers: in O^T = V^T P^T the
// k index of MFMA step r of key block kb is lane group grp <-> key 16 kb + 4 grp + r, so a lane's B operand is its own w[kb][r] and the A
// operand is V[16 kb + 4 grp + r][16 db + col] from LDS.  The quotient by the row sum is taken once per output element, at the end.
//
// Every order is fixed and there are no atomics on out: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_launch.h"
#include "mvnerf_mfma.h"
#include "mvnerf_vit.h"

namespace mvnerf {

namespace {

constexpr int kAtThreads = 256;
constexpr int kAtMaxKeys = 256;                               // 16 key blocks of 16: the logits of one query block stay in registers
constexpr int kAtKeyBlocks = kAtMaxKeys / 16;
constexpr int kAtPad = 4;                                     // floats behind each staged key row

constexpr int at_lds_bytes(int n, int d) { return 2 * ((n + 15) / 16 * 16) * (d + kAtPad) * (int)sizeof(float); }
static_assert(at_lds_bytes(kAtMaxKeys, 64) <= 160 * 1024, "K and V of one head fit the LDS");

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <int kD>
__global__ __launch_bounds__(kAtThreads) void attention_kernel(const float* __restrict__ qkv, int n, int heads, float scale,
                                                               float* __restrict__ out, unsigned* __restrict__ amax_out, int q_splits) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ unsigned slot;
    constexpr int kStride = kD + kAtPad, kQuads = kD / 4, kDb = kD / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const int bh = blockIdx.x / q_splits, qs = blockIdx.x % q_splits;
    const int b = bh / heads, h = bh % heads;
    const int nkb = (n + 15) / 16, n_pad = nkb * 16;
    float* ks = reinterpret_cast<float*>(lds_raw);
    float* vs = ks + n_pad * kStride;
    const size_t tok = (size_t)3 * heads * kD;                               // floats per token
    const float* base = qkv + (size_t)b * n * tok + (size_t)h * kD;          // q of token 0; k and v lie heads d and 2 heads d behind

    if (tid == 0) slot = 0;
    for (int item = tid; item < n_pad * kQuads; item += kAtThreads) {        // keys past n: zeros, nothing is read
        const int r = item / kQuads, qd = item % kQuads;
        f32x4 k4 = {0.0f, 0.0f, 0.0f, 0.0f}, v4 = k4;
        if (r < n) {
            const float* src = base + r * tok + 4 * qd;
            k4 = *reinterpret_cast<const f32x4*>(src + heads * kD);
            v4 = *reinterpret_cast<const f32x4*>(src + 2 * heads * kD);
        }
        *reinterpret_cast<f32x4*>(ks + r * kStride + 4 * qd) = k4;
        *reinterpret_cast<f32x4*>(vs + r * kStride + 4 * qd) = v4;
    }
    __syncthreads();

    const int qb = qs * 4 + wave;                                            // this wave's block of 16 queries
    unsigned top = 0;
    if (qb < nkb) {                                                          // (wave-uniform)
        const int query = qb * 16 + col;
        f32x4 q[kDb];
#pragma unroll
        for (int j = 0; j < kDb; ++j) {
            q[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (query < n) q[j] = *reinterpret_cast<const f32x4*>(base + query * tok + 16 * j + 4 * grp);
        }
        // logits: s[kb][r] is query `col` against key 16 kb + 4 grp + r
        const float minus_inf = __builtin_bit_cast(float, 0xff800000u);
        f32x4 s[kAtKeyBlocks];
        float top_s = minus_inf;
#pragma unroll
        for (int kb = 0; kb < kAtKeyBlocks; ++kb) {
            s[kb] = f32x4{minus_inf, minus_inf, minus_inf, minus_inf};
            if (kb < nkb) {
                f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < kDb; ++j) {
                    const f32x4 k4 = *reinterpret_cast<const f32x4*>(ks + (16 * kb + col) * kStride + 16 * j + 4 * grp);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = mfma4(k4[e], q[j][e], acc);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float logit = acc[r] * scale;
                    s[kb][r] = 16 * kb + 4 * grp + r < n ? logit : minus_inf;
                    top_s = fmaxf(top_s, s[kb][r]);
                }
            }
        }
        top_s = fmaxf(top_s, __shfl_xor(top_s, 16));
        top_s = fmaxf(top_s, __shfl_xor(top_s, 32));
        float total = 0.0f;
#pragma unroll
        for (int kb = 0; kb < kAtKeyBlocks; ++kb)
            if (kb < nkb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float w = vit_softmax_weight(s[kb][r], top_s);
                    s[kb][r] = w;
                    total = total + w;
                }
        total = total + __shfl_xor(total, 16);
        total = total + __shfl_xor(total, 32);

        // O^T: o[db][r] is channel 16 db + 4 grp + r of query `col`
        f32x4 o[kDb];
#pragma unroll
        for (int db = 0; db < kDb; ++db) o[db] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kb = 0; kb < kAtKeyBlocks; ++kb)
            if (kb < nkb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float* vrow = vs + (16 * kb + 4 * grp + r) * kStride + col;
#pragma unroll
                    for (int db = 0; db < kDb; ++db) o[db] = mfma4(vrow[16 * db], s[kb][r], o[db]);
                }
        if (query < n) {
            float* dst = out + ((size_t)b * n + query) * heads * kD + (size_t)h * kD + 4 * grp;
#pragma unroll
            for (int db = 0; db < kDb; ++db) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] = o[db][r] / total;
                    const unsigned bits = __builtin_bit_cast(unsigned, (float)v[r]) & 0x7fffffffu;
                    top = bits > top ? bits : top;
                }
                *reinterpret_cast<f32x4*>(dst + 16 * db) = v;
            }
        }
    }
    if (amax_out) {                                              // (the same in every thread; slot was zeroed before the first barrier)
        atomicMax(&slot, top);
        __syncthreads();
        if (tid == 0) atomicMax(amax_out, slot);
    }
}

}  // namespace

}  // namespace mvnerf

extern "C" {

int mvnerf_attention_tokens(const float* qkv, int B, int n, int heads, int d, float scale, float* out, float* amax_out, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_attention_tokens";
    if (!qkv || !out) return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who, !qkv ? "qkv" : "out");
    if (B <= 0 || heads <= 0 || n <= 0) return api_fail(MVNERF_E_ARG, "%s: B=%d n=%d heads=%d", who, B, n, heads);
    if (!(scale == scale) || scale - scale != 0.0f) return api_fail(MVNERF_E_ARG, "%s: scale=%g (a finite number)", who, (double)scale);
    if (d != 16 && d != 32 && d != 64) return api_fail(MVNERF_E_SHAPE, "%s: d=%d (16, 32 or 64)", who, d);
    if (n > kAtMaxKeys) return api_fail(MVNERF_E_SHAPE, "%s: n=%d (at most %d tokens)", who, n, kAtMaxKeys);
    const int q_splits = ((n + 15) / 16 + 3) / 4;
    const long blocks = (long)B * heads * q_splits;
    if (blocks > 0x7fffffffL)
        return api_fail(MVNERF_E_SHAPE, "%s: B=%d n=%d heads=%d d=%d (at most 2^31 - 1 workgroups)", who, B, n, heads, d);
    if (!aligned16(qkv) || !aligned16(out)) return api_fail(MVNERF_E_ALIGN, "%s: %s must be 16-byte aligned", who, !aligned16(qkv) ? "qkv" : "out");
    if (!aligned4(amax_out)) return api_fail(MVNERF_E_ALIGN, "%s: amax_out must be 4-byte aligned", who);
    static DeviceSetup setup;
    MV_HIP(device_setup(setup, {{attention_kernel<16>, at_lds_bytes(kAtMaxKeys, 16)}, {attention_kernel<32>, at_lds_bytes(kAtMaxKeys, 32)},
                                {attention_kernel<64>, at_lds_bytes(kAtMaxKeys, 64)}}), who);
    auto* kernel = d == 16 ? attention_kernel<16> : d == 32 ? attention_kernel<32> : attention_kernel<64>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kAtThreads), at_lds_bytes(n, d), static_cast<hipStream_t>(stream), qkv, n, heads,
                       scale, out, reinterpret_cast<unsigned*>(amax_out), q_splits);
    return hip_status(hipGetLastError(), who);
}

}  // extern "C"
