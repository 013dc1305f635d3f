// Per-pose scalar math of the grasp-pose optimiser (DNGFOptimizer, src/lib/lmvnerf/grasp_optimizer.py:28-184), usable from device
// code (hipcc, pose_ops.hip) and from a host build (gcc, tests/cpu_pose) so the same source is checked on the CPU.
//
//   pose -> (R, t)            compute_matrices (:113-124): tfg from_quaternion (x, y, z, w, q used as given) or the 6d form (both halves
//                             normalised, third column their cross product, not orthogonalised)
//   offset -> point, dir      LanguageNeRF._query_points (model_v4.py:222-226): point = R t_o + t, dir = R z_o (z_o = the offset's z axis)
//   12 sums -> (d_t, d_rot)   G = sum_rows dp (x) t_o + dd (x) z_o = dL/dR, g_t = sum_rows dp, then the closed-form derivative of R(rot)
//   Adam + post_process       optimize() = clip-by-value then tf.keras.optimizers.Adam (TF 2.11 form) with ExponentialDecay(decay_steps=1),
//                             then post_process (:126-139): clip t to the workspace bounds, normalise q or each half of the 6d vector
//
// Arithmetic: the library is compiled with -ffp-contract=off (one rounding per written operation, as mvnerf_math.h); sums run in the
// order written here.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define MVP_HD __host__ __device__ __forceinline__
#else
#define MVP_HD static inline
#endif

namespace mvnerf {
namespace pose {

constexpr int kRepQuaternion = 0;
constexpr int kRep6d = 1;

MVP_HD int rot_dim(int rep) { return rep == kRepQuaternion ? 4 : 6; }

// R (row-major 3x3) of one pose.  rot: 4 (x, y, z, w) or 6 ([r1 | r2]) floats.
MVP_HD void rotation(int rep, const float* rot, float* R) {
    if (rep == kRepQuaternion) {
        // tensorflow_graphics rotation_matrix_3d.from_quaternion, term for term (thesis_clip_nerf_amd/lmvnerf.py rotation_from_quaternion)
        const float x = rot[0], y = rot[1], z = rot[2], w = rot[3];
        const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
        const float twx = tx * w, twy = ty * w, twz = tz * w;
        const float txx = tx * x, txy = ty * x, txz = tz * x;
        const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
        R[0] = 1.0f - (tyy + tzz); R[1] = txy - twz;          R[2] = txz + twy;
        R[3] = txy + twz;          R[4] = 1.0f - (txx + tzz); R[5] = tyz - twx;
        R[6] = txz - twy;          R[7] = tyz + twx;          R[8] = 1.0f - (txx + tyy);
    } else {
        float c[6];
        for (int h = 0; h < 2; ++h) {
            const float* a = rot + 3 * h;
            const float n = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);       // tf.linalg.normalize: x / ||x||
            c[3 * h] = a[0] / n; c[3 * h + 1] = a[1] / n; c[3 * h + 2] = a[2] / n;
        }
        const float* r1 = c;
        const float* r2 = c + 3;
        const float r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
        for (int i = 0; i < 3; ++i) { R[3 * i] = r1[i]; R[3 * i + 1] = r2[i]; R[3 * i + 2] = r3[i]; }
    }
}

// offset o (row-major 4x4, last row 0 0 0 1) of transforms_to_check -> its translation t_o and z axis z_o
MVP_HD void offset_parts(const float* off, float* ot, float* oz) {
    for (int i = 0; i < 3; ++i) { ot[i] = off[4 * i + 3]; oz[i] = off[4 * i + 2]; }
}

// query point and direction of (pose, offset): p = R t_o + t, d = R z_o
MVP_HD void query_point(const float* R, const float* t, const float* ot, const float* oz, float* p, float* d) {
    for (int i = 0; i < 3; ++i) {
        p[i] = ((R[3 * i] * ot[0] + R[3 * i + 1] * ot[1]) + R[3 * i + 2] * ot[2]) + t[i];
        d[i] = (R[3 * i] * oz[0] + R[3 * i + 1] * oz[1]) + R[3 * i + 2] * oz[2];
    }
}

// acc[0..8] += dp (x) t_o + dd (x) z_o (row-major G), acc[9..11] += dp
MVP_HD void accumulate_row(float* acc, const float* dp, const float* dd, const float* ot, const float* oz) {
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) acc[3 * i + k] += dp[i] * ot[k] + dd[i] * oz[k];
        acc[9 + i] += dp[i];
    }
}

// (G = dL/dR, g_t = dL/dt) -> scale * (d_t, d_rot)
MVP_HD void pose_vjp(int rep, const float* rot, const float* acc, float scale, float* d_t, float* d_rot) {
    const float* G = acc;
    for (int i = 0; i < 3; ++i) d_t[i] = scale * acc[9 + i];
    if (rep == kRepQuaternion) {
        const float x = rot[0], y = rot[1], z = rot[2], w = rot[3];
        const float s01 = G[1] + G[3], s02 = G[2] + G[6], s12 = G[5] + G[7];      // symmetric parts
        const float a01 = G[3] - G[1], a02 = G[2] - G[6], a12 = G[7] - G[5];      // antisymmetric parts
        d_rot[0] = scale * (2.0f * ((y * s01 + z * s02) + w * a12) - 4.0f * (x * (G[4] + G[8])));
        d_rot[1] = scale * (2.0f * ((x * s01 + w * a02) + z * s12) - 4.0f * (y * (G[0] + G[8])));
        d_rot[2] = scale * (2.0f * ((w * a01 + x * s02) + y * s12) - 4.0f * (z * (G[0] + G[4])));
        d_rot[3] = scale * (2.0f * ((z * a01 + y * a02) + x * a12));
    } else {
        float c[6], n[2];
        for (int h = 0; h < 2; ++h) {
            const float* a = rot + 3 * h;
            n[h] = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
            c[3 * h] = a[0] / n[h]; c[3 * h + 1] = a[1] / n[h]; c[3 * h + 2] = a[2] / n[h];
        }
        const float* r1 = c;
        const float* r2 = c + 3;
        const float g3[3] = {G[2], G[5], G[8]};
        // L = g3 . (r1 x r2): dL/dr1 = r2 x g3, dL/dr2 = g3 x r1
        float g[6] = {G[0] + (r2[1] * g3[2] - r2[2] * g3[1]), G[3] + (r2[2] * g3[0] - r2[0] * g3[2]), G[6] + (r2[0] * g3[1] - r2[1] * g3[0]),
                      G[1] + (g3[1] * r1[2] - g3[2] * r1[1]), G[4] + (g3[2] * r1[0] - g3[0] * r1[2]), G[7] + (g3[0] * r1[1] - g3[1] * r1[0])};
        for (int h = 0; h < 2; ++h) {                       // through r = a / ||a||: (g - r (r . g)) / ||a||
            const float* r = c + 3 * h;
            const float* gh = g + 3 * h;
            const float rg = (r[0] * gh[0] + r[1] * gh[1]) + r[2] * gh[2];
            for (int i = 0; i < 3; ++i) d_rot[3 * h + i] = scale * ((gh[i] - r[i] * rg) / n[h]);
        }
    }
}

// ---- forward mode (LanguageNeRF.train_step, model_v4.py:290-322: the loss on d prediction / d pose is differentiated through the pose
// map a second time; the pose VJP is linear in its cotangent, so that derivative is this product) ----
// dR (row-major 3x3) = the derivative of rotation(rep, rot) along c_rot.
MVP_HD void rotation_jvp(int rep, const float* rot, const float* c_rot, float* dR) {
    if (rep == kRepQuaternion) {
        // term for term the derivative of the tfg form above, q as given (not normalised)
        const float x = rot[0], y = rot[1], z = rot[2], w = rot[3];
        const float dx = c_rot[0], dy = c_rot[1], dz = c_rot[2], dw = c_rot[3];
        const float dxx = 4.0f * (x * dx), dyy = 4.0f * (y * dy), dzz = 4.0f * (z * dz);          // d(2 x x) ...
        const float dxy = 2.0f * (x * dy + y * dx), dxz = 2.0f * (x * dz + z * dx), dyz = 2.0f * (y * dz + z * dy);
        const float dwx = 2.0f * (w * dx + x * dw), dwy = 2.0f * (w * dy + y * dw), dwz = 2.0f * (w * dz + z * dw);
        dR[0] = -(dyy + dzz); dR[1] = dxy - dwz;    dR[2] = dxz + dwy;
        dR[3] = dxy + dwz;    dR[4] = -(dxx + dzz); dR[5] = dyz - dwx;
        dR[6] = dxz - dwy;    dR[7] = dyz + dwx;    dR[8] = -(dxx + dyy);
    } else {
        float c[6], dc[6];
        for (int h = 0; h < 2; ++h) {                       // r = a / ||a||: dr = (da - r (r . da)) / ||a||
            const float* a = rot + 3 * h;
            const float* da = c_rot + 3 * h;
            const float n = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
            float* r = c + 3 * h;
            r[0] = a[0] / n; r[1] = a[1] / n; r[2] = a[2] / n;
            const float rd = (r[0] * da[0] + r[1] * da[1]) + r[2] * da[2];
            for (int i = 0; i < 3; ++i) dc[3 * h + i] = (da[i] - r[i] * rd) / n;
        }
        const float* r1 = c;
        const float* r2 = c + 3;
        const float* d1 = dc;
        const float* d2 = dc + 3;
        // r3 = r1 x r2: dr3 = dr1 x r2 + r1 x dr2
        const float d3[3] = {(d1[1] * r2[2] - d1[2] * r2[1]) + (r1[1] * d2[2] - r1[2] * d2[1]),
                             (d1[2] * r2[0] - d1[0] * r2[2]) + (r1[2] * d2[0] - r1[0] * d2[2]),
                             (d1[0] * r2[1] - d1[1] * r2[0]) + (r1[0] * d2[1] - r1[1] * d2[0])};
        for (int i = 0; i < 3; ++i) { dR[3 * i] = d1[i]; dR[3 * i + 1] = d2[i]; dR[3 * i + 2] = d3[i]; }
    }
}

// tangents of query_point: t_p = dR t_o + c_t, t_d = dR z_o (the same sums as query_point, R -> dR, t -> c_t)
MVP_HD void query_point_jvp(const float* dR, const float* c_t, const float* ot, const float* oz, float* tp, float* td) {
    query_point(dR, c_t, ot, oz, tp, td);
}

// ---- the optimiser (src/utils/optimization.py:40-69; TF 2.11 keras Adam, ExponentialDecay(init, decay_steps=1, rate, staircase=False)) ----
struct AdamConfig {
    float lr0[2], decay[2];          // per variable: 0 = translations, 1 = rotations
    float beta1, beta2, eps, clip;   // clip <= 0: no clip-by-value
    int clip_translation;
    float lo[3], hi[3];              // workspace bounds per axis
};

// step k = 1, 2, ... of a variable: lr = lr0 rate^(k-1), alpha = lr sqrt(1 - beta2^k) / (1 - beta1^k); in double, rounded once
MVP_HD float adam_alpha(float lr0, float decay, int k, float beta1, float beta2) {
    const double lr = (double)lr0 * pow((double)decay, (double)(k - 1));
    return (float)(lr * sqrt(1.0 - pow((double)beta2, (double)k)) / (1.0 - pow((double)beta1, (double)k)));
}

// clip-by-value, then m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); x -= alpha m / (sqrt(v) + eps)
MVP_HD void adam_update(float* x, float* m, float* v, const float* g, int n, float alpha, const AdamConfig& c) {
    for (int i = 0; i < n; ++i) {
        float gi = g[i];
        if (c.clip > 0.0f) gi = fminf(fmaxf(gi, -c.clip), c.clip);
        m[i] += (gi - m[i]) * (1.0f - c.beta1);
        v[i] += (gi * gi - v[i]) * (1.0f - c.beta2);
        x[i] -= (m[i] * alpha) / (sqrtf(v[i]) + c.eps);
    }
}

MVP_HD void normalize3(float* a) {
    const float n = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    a[0] = a[0] / n; a[1] = a[1] / n; a[2] = a[2] / n;
}

// post_process (grasp_optimizer.py:126-139), applied after every step whichever variables were trained
MVP_HD void post_process(int rep, const AdamConfig& c, float* t, float* rot) {
    if (c.clip_translation)
        for (int i = 0; i < 3; ++i) t[i] = fminf(fmaxf(t[i], c.lo[i]), c.hi[i]);
    if (rep == kRepQuaternion) {
        const float n = sqrtf(((rot[0] * rot[0] + rot[1] * rot[1]) + rot[2] * rot[2]) + rot[3] * rot[3]);
        for (int i = 0; i < 4; ++i) rot[i] = rot[i] / n;
    } else {
        normalize3(rot);
        normalize3(rot + 3);
    }
}

// One optimisation step of one pose.  flags[v] != 0: variable v (0 = t, 1 = rot) is trained and its own counter count[v] advances.
MVP_HD void adam_step_pose(int rep, const AdamConfig& c, const int* flags, int* count_t, int* count_r, const float* g_t, const float* g_r,
                           float* m_t, float* v_t, float* m_r, float* v_r, float* t, float* rot) {
    if (flags[0]) {
        const int k = *count_t + 1;
        *count_t = k;
        adam_update(t, m_t, v_t, g_t, 3, adam_alpha(c.lr0[0], c.decay[0], k, c.beta1, c.beta2), c);
    }
    if (flags[1]) {
        const int k = *count_r + 1;
        *count_r = k;
        adam_update(rot, m_r, v_r, g_r, rot_dim(rep), adam_alpha(c.lr0[1], c.decay[1], k, c.beta1, c.beta2), c);
    }
    post_process(rep, c, t, rot);
}

}  // namespace pose
}  // namespace mvnerf
