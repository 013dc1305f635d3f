// Device helpers shared by the fused field kernels (field_eval.hip: inference / training forward; query_ops.hip:
// forward-mode tangent kernel): accumulator-order bias loads and row stores, the swizzled wave-private LDS stage; the sample
// front end of the kernels on the 32x32 lane mapping (field_eval.hip, field_eval_split.hip, field_eval_bf16.hip); and the
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

// the same load for kernels whose waves share a weight ring: the add is pinned to scalar v_add_f32 - left to the compiler it becomes
// v_pk_add_f32, which costs the matrix pipe of the partner wave far more than two v_add_f32 (MI355X_MICROARCH.md, fillers beside MFMAs)
template <bool kAdd>
__device__ __forceinline__ void bias_acc(const float* __restrict__ bperm, int h, f32x16 (&acc)[4]) {
    const f32x4* p = reinterpret_cast<const f32x4*>(bperm + h * 64);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = p[nb * 4 + q];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (kAdd) {
                    float r = acc[nb][4 * q + c];
                    asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(r), "v"(v[c]));
                    acc[nb][4 * q + c] = r;
                } else {
                    acc[nb][4 * q + c] = v[c];
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

// ---- the sample front end on the 32x32 lane mapping: lane = (sample j = lane & 31, half h = lane >> 5) ----
// Every kernel that starts a tile this way calls these routines, in its own order (the order is what the register allocator sees);
// the parity contract of mvnerf_math.h - the same fp32 operations in every kernel - then holds by construction.  The 16x16x32
// kernels (field_eval_split16_impl.h, field_eval_bf16x.hip) map lanes differently and keep their own front end, as do the tangent
// kernel (query_ops.hip) and the backward kernels (train_ops.hip), which need the intermediates these routines do not keep.
struct LaneSample {
    long g;              // sample index in [0, total), clamped: lanes past the end shadow the last sample
    bool valid;          // the lane's own sample of the wave's own tile: only then does it store
    int ray, sidx, b;    // global ray in [0, B*R), sample on the ray, scene
    float wx, wy, wz;    // world point o + z d
};

// tile: the wave's tile, already clamped to n_tiles - 1 where tile_ok is false (idle waves shadow the last tile)
__device__ __forceinline__ LaneSample lane_sample(const FieldParams& p, long tile, bool tile_ok, int j) {
    LaneSample s;
    s.g = tile * kTile + j;
    s.valid = tile_ok && s.g < p.total;
    if (s.g >= p.total) s.g = p.total - 1;
    s.ray = (int)(s.g / p.S);
    s.sidx = (int)(s.g - (long)s.ray * p.S);
    s.b = s.ray / p.R;
    const float ox = p.rays_o[3 * s.ray + 0], oy = p.rays_o[3 * s.ray + 1], oz = p.rays_o[3 * s.ray + 2];
    const float dx = p.rays_d[3 * s.ray + 0], dy = p.rays_d[3 * s.ray + 1], dz = p.rays_d[3 * s.ray + 2];
    const float zz = p.z[s.g];
    s.wx = ox + zz * dx, s.wy = oy + zz * dy, s.wz = oz + zz * dz;        // mul, then add (no FMA)
    return s;
}

struct ViewSample {
    float cam[4];        // camera-space point
    float pxl, pyl;      // pixel
    Taps tp;
    int tl;              // top-left texel of the four taps, index into (B*V, H, W)
    long vray, vrow;     // rows in a (B*V, R, ..) and a (B*V, R, S, ..) tensor
};

__device__ __forceinline__ ViewSample view_sample(const FieldParams& p, const LaneSample& s, int bv) {
    ViewSample vs;
    const float* E = p.einv + 16 * bv;
#pragma unroll
    for (int r = 0; r < 4; ++r) vs.cam[r] = row_dot4(E, r, s.wx, s.wy, s.wz, 1.0f);
    pixel_from_cam(p.k4 + 16 * bv, vs.cam, &vs.pxl, &vs.pyl);
    vs.tp = bilinear_taps(vs.pxl, vs.pyl, p.H, p.W);
    vs.tl = (bv * p.H + vs.tp.y0) * p.W + vs.tp.x0;
    vs.vray = (long)bv * p.R + (s.ray - s.b * p.R);
    vs.vrow = vs.vray * p.S + s.sidx;
    return vs;
}

// the optional return_taps / return_pix outputs, by the lower half-wave's valid lanes
__device__ __forceinline__ void store_tap_idx(const FieldParams& p, const ViewSample& vs) {
    if (!p.tap_idx) return;
    int4 t4 = make_int4(vs.tl, vs.tl + 1, vs.tl + p.W, vs.tl + p.W + 1);
    *reinterpret_cast<int4*>(p.tap_idx + 4 * vs.vrow) = t4;
}
__device__ __forceinline__ void store_pix(const FieldParams& p, const ViewSample& vs) {
    if (!p.pix) return;
    p.pix[2 * vs.vrow + 0] = vs.pxl;
    p.pix[2 * vs.vrow + 1] = vs.pyl;
}

// training mode: the view tile of a multi-view pass, (b V + v) tiles_per_b + k (all 32 samples of a tile share b because
// R*S % 32 == 0 when V > 1)
__device__ __forceinline__ long view_tile(const FieldParams& p, long tile, int b, int bv) {
    return (long)bv * (p.n_tiles / p.B) + (tile - (long)b * (p.n_tiles / p.B));
}

// PE(cam xyz) as the B operands of k-steps 0..29 (lower half-wave sin, upper cos)
__device__ __forceinline__ void pe_cam_xyz(const float (&cam)[4], int h, float (&pe)[32]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float a0 = cam[d] * 3.14159274101257324f;
        float sk = 0.0f, ck = 0.0f;
#pragma unroll
        for (int k = 0; k < kNFreq; ++k) {
            // fl32(x * fl32(pi*2^k)) == 2^k * fl32(x * fl32(pi)) exactly, so octave k is the k-fold double
            // angle of octave 0.  Accurate sin/cos at k = 0 and k = 5, double-angle steps in between (error
            // x16 at most: ~2e-6 absolute against the 1e-4 bar; the op-level position_encoding is exact).
            if (k == 0 || k == 5) {
                sincos_f32(a0 * (float)(1 << k), &sk, &ck);
            } else {
                const float s2 = sk + sk;
                const float cn = fmaf(-s2, sk, 1.0f);              // cos 2t = 1 - 2 sin^2 t
                sk = s2 * ck;                                      // sin 2t = 2 sin t cos t
                ck = cn;
            }
            pe[d * 10 + k] = h ? ck : sk;
        }
    }
}

// rgb taps of the lane's own sample, normalised 2*img-1 before the lerp (model_v0.py:120): B operands of k-steps 30, 31
__device__ __forceinline__ void rgb_inputs(const float* __restrict__ images, int tl, int W, const Taps& tp, int h, float (&pe)[32]) {
    const float* img = images + 3 * (long)tl;
    float rgbv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = img[c] * 2.0f - 1.0f, bq = img[3 + c] * 2.0f - 1.0f;
        const float cq = img[3 * W + c] * 2.0f - 1.0f, dq = img[3 * W + 3 + c] * 2.0f - 1.0f;
        rgbv[c] = bilerp(a, bq, cq, dq, tp.ax, tp.ay);
    }
    pe[30] = h ? rgbv[1] : rgbv[0];
    pe[31] = h ? 0.0f : rgbv[2];
}

// four channels of the four taps: the bilinear form of tfa (lerp x, then y), each lerp as one FMA after the difference (6 instead
// of 9 vector instructions per channel)
__device__ __forceinline__ f32x4 lerp_taps(f32x4 vtl, f32x4 vtr, f32x4 vbl, f32x4 vbr, float ax, float ay) {
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float top = fmaf(ax, vtr[c] - vtl[c], vtl[c]);
        const float bot = fmaf(ax, vbr[c] - vbl[c], vbl[c]);
        o[c] = fmaf(ay, bot - top, top);
    }
    return o;
}

// read-out activations (layers.py:395-396) and the (rgb, sigma) row of sample g
__device__ __forceinline__ void store_readout(float* __restrict__ rgbs, long g, float o0, float o1, float o2, float o3) {
    f32x4 out;
    out[0] = sigmoid_f32(o0);
    out[1] = sigmoid_f32(o1);
    out[2] = sigmoid_f32(o2);
    out[3] = softplus_f32(o3);
    *reinterpret_cast<f32x4*>(rgbs + 4 * g) = out;
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
