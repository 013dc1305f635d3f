// Device helpers shared by the fused field kernels (field_eval.hip: inference / training forward; query_ops.hip:
// forward-mode tangent kernel): accumulator-order bias loads and row stores, the swizzled wave-private LDS stage; and the
// per-(view, ray) layer-0 seed row, shared by dir_bias_kernel and the split16 kernels that form their rays' rows themselves.
#pragma once

#include "mvnerf_kernels.h"
#include "mvnerf_math.h"
#include "mvnerf_mfma.h"
#include "mvnerf_pack.h"

namespace mvnerf {

constexpr int kTile = 32;            // samples per wavefront (MFMA N dimension)
constexpr int kStageRow = 128;       // floats per staged sample row (half of the 256 channels)

template <bool kAdd>
__device__ __forceinline__ void bias_to_acc(const float* __restrict__ bperm, int h, f32x16 (&acc)[4]) {
    const f32x4* p = reinterpret_cast<const f32x4*>(bperm + h * 64);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = p[nb * 4 + q];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (kAdd) acc[nb][4 * q + c] = acc[nb][4 * q + c] + v[c];
                else acc[nb][4 * q + c] = v[c];
            }
        }
    }
}

// lane (j,h) holds features 32*nb + 8*q + 4*h + {0..3} of sample j in registers 4q..4q+3 of block nb
__device__ __forceinline__ void store_acc(float* __restrict__ row128, int h, const f32x16 (&x)[4]) {
    float* e = row128 + 4 * h;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 v4 = {x[nb][4 * q], x[nb][4 * q + 1], x[nb][4 * q + 2], x[nb][4 * q + 3]};
            *reinterpret_cast<f32x4*>(e + 32 * nb + 8 * q) = v4;
        }
}

__device__ __forceinline__ int stage_offset(int row, int chunk) {      // floats; XOR swizzle on 16-B chunks
    return row * kStageRow + ((chunk ^ (row & 15)) << 2);
}

// read-only kernel inputs at a wave-uniform address, read through the constant address space: scalar loads
using cfloat = const __attribute__((address_space(4))) float;

// ---- per-(view, ray) layer-0 seed: b0 + W0[60:120]^T PE(cam dir)  (the direction is constant along a ray) ----
// One wavefront forms the row of ray r (inside its scene) under view bv = b*V + v and stores it at p.dir_bias + 128 (bv R + r) in
// accumulator order [h][nb][r], so that a field kernel loads it like a bias.  wd: the plain copy of W0 rows 60..119, [60][128], with
// b0[128] behind it (p.net + kPackW0Dir, or a copy of those 30 KiB + 512 B in LDS).  bv and r are wave-uniform (the caller's readfirstlane):
// the ray and the view's matrix come through scalar loads, which no vector-memory wait of the caller orders.
__device__ __forceinline__ void dir_seed_row(const FieldParams& p, int bv, int r, int lane, const float* wd) {
    const long ray = (long)(bv / p.V) * p.R + r;
    const cfloat* rd = (const cfloat*)(p.rays_d + 3 * ray);
    const cfloat* Ec = (const cfloat*)(p.einv + 16 * bv);
    const float dx = rd[0], dy = rd[1], dz = rd[2];
    float E[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) E[i] = Ec[i];
    // lane m < 60 evaluates PE feature m = d*20 + 2k + f (nerf_utils.py:124 layout) of cam dir (Q3: w = 1)
    const int m = lane < 60 ? lane : 59;
    const int d = m / 20, k = (m % 20) >> 1, f = m & 1;
    const float cd0 = row_dot4(E, 0, dx, dy, dz, 1.0f), cd1 = row_dot4(E, 1, dx, dy, dz, 1.0f), cd2 = row_dot4(E, 2, dx, dy, dz, 1.0f);
    const float cd = d == 0 ? cd0 : (d == 1 ? cd1 : cd2);
    float sv, cv;
    sincos_f32(cd * (3.14159274101257324f * (float)(1 << k)), &sv, &cv);
    const float mine = f ? cv : sv;
    float a0 = wd[kPackB0Plain - kPackW0Dir + lane], a1 = wd[kPackB0Plain - kPackW0Dir + 64 + lane];       // b0, behind the 60 rows
    for (int mm = 0; mm < 60; ++mm) {
        const float pv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine), mm));
        a0 = fmaf(pv, wd[mm * 128 + lane], a0);
        a1 = fmaf(pv, wd[mm * 128 + 64 + lane], a1);
    }
    float* out = p.dir_bias + 128 * ((long)bv * p.R + r);
    out[acc_slot(lane)] = a0;
    out[acc_slot(64 + lane)] = a1;
}

}  // namespace mvnerf
