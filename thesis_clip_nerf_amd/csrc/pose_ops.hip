// The pose side of the grasp-pose optimiser (DNGFOptimizer.optimize_pose, src/lib/lmvnerf/grasp_optimizer.py:158-184; the loop of
// src/utils/optimization.py:40-152) as three launches per step around the trunk and the read-out:
//
//   pose_query_points : (t, rot) -> the query points and directions of every (pose, gripper offset), written once per scene (B copies),
//                       in the query order (pose, offset) of LanguageNeRF._query_points.  One thread per (pose, offset).
//   pose_query_vjp    : (d_points, d_dirs) -> (d_t, d_rot).  One wavefront per pose: each lane sums its rows of the B * n5 into the 12
//                       numbers (G = dL/dR, dL/dt), a fixed butterfly combines the lanes (no atomics: the result is the same bits from run
//                       to run), lane 0 applies the closed-form derivative of R(rot).
//   pose_query_jvp    : (c_t, c_rot) -> (t_points, t_dirs), the forward-mode product of pose_query_points with its structure (one thread per
//                       (pose, offset)); what LanguageNeRF.train_step's nested tape takes of the pose map (csrc/language_api.hip).
//   pose_adam_step    : clip-by-value, Keras Adam with the exponentially decayed rate computed on the device from per-pose step counters,
//                       post_process.  One thread per pose owns that pose's counters, so they advance without a race; which variables
//                       train comes from a device-resident flag pair, so one captured step serves both phases.
//
// The math per pose is mvnerf_pose.h (also built for the host by tests/cpu_pose, tests/cpu_language).  All are tiny next to the trunk passes (bytes:
// ~2 x B * P * n5 * 24 per step); the point is to replace ~60 torch launches per step and keep the whole step capturable.
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_pose.h"

namespace mvnerf {

namespace {

__global__ void pose_query_points_kernel(const float* __restrict__ t, const float* __restrict__ rot, int rep,
                                         const float* __restrict__ offsets, int P, int n5, int B, long ld, float* __restrict__ points,
                                         float* __restrict__ dirs) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)P * n5) return;
    const int p = (int)(idx / n5), o = (int)(idx % n5);
    const int rd = pose::rot_dim(rep);
    float r[6], R[9], tt[3], ot[3], oz[3], pt[3], dr[3];
    for (int i = 0; i < rd; ++i) r[i] = rot[(long)p * rd + i];
    for (int i = 0; i < 3; ++i) tt[i] = t[(long)p * 3 + i];
    pose::rotation(rep, r, R);
    pose::offset_parts(offsets + 16 * o, ot, oz);
    pose::query_point(R, tt, ot, oz, pt, dr);
    for (int b = 0; b < B; ++b) {
        const long row = (long)b * ld + idx;
        for (int i = 0; i < 3; ++i) {
            points[row * 3 + i] = pt[i];
            dirs[row * 3 + i] = dr[i];
        }
    }
}

// The forward-mode product of pose_query_points_kernel, same structure: one thread per (pose, offset) forms dR of its pose along c_rot and
// writes t_point = dR t_o + c_t, t_dir = dR z_o once per scene.  Rows past P * n5 of a scene are left alone.
__global__ void pose_query_jvp_kernel(const float* __restrict__ rot, int rep, const float* __restrict__ offsets, const float* __restrict__ c_t,
                                      const float* __restrict__ c_rot, int P, int n5, int B, long ld, float* __restrict__ t_points,
                                      float* __restrict__ t_dirs) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)P * n5) return;
    const int p = (int)(idx / n5), o = (int)(idx % n5);
    const int rd = pose::rot_dim(rep);
    float r[6], cr[6], dR[9], ct[3], ot[3], oz[3], tp[3], td[3];
    for (int i = 0; i < rd; ++i) { r[i] = rot[(long)p * rd + i]; cr[i] = c_rot[(long)p * rd + i]; }
    for (int i = 0; i < 3; ++i) ct[i] = c_t[(long)p * 3 + i];
    pose::rotation_jvp(rep, r, cr, dR);
    pose::offset_parts(offsets + 16 * o, ot, oz);
    pose::query_point_jvp(dR, ct, ot, oz, tp, td);
    for (int b = 0; b < B; ++b) {
        const long row = (long)b * ld + idx;
        for (int i = 0; i < 3; ++i) {
            t_points[row * 3 + i] = tp[i];
            t_dirs[row * 3 + i] = td[i];
        }
    }
}

constexpr int kVjpWaves = 4;    // poses per 256-thread block

__global__ __launch_bounds__(64 * kVjpWaves) void pose_query_vjp_kernel(const float* __restrict__ rot, int rep,
                                                                          const float* __restrict__ offsets,
                                                                          const float* __restrict__ d_points,
                                                                          const float* __restrict__ d_dirs, int P, int n5, int B, long ld,
                                                                          float scale, float* __restrict__ d_t, float* __restrict__ d_rot) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * kVjpWaves + (threadIdx.x >> 6);
    if (p >= P) return;                                  // whole wave
    float acc[12];
    for (int i = 0; i < 12; ++i) acc[i] = 0.0f;
    const int rows = B * n5;
    for (int j = lane; j < rows; j += 64) {              // lane-strided rows, in the same order every run
        const int b = j / n5, o = j % n5;
        const long row = (long)b * ld + (long)p * n5 + o;
        float dp[3], dd[3], ot[3], oz[3];
        for (int i = 0; i < 3; ++i) { dp[i] = d_points[row * 3 + i]; dd[i] = d_dirs[row * 3 + i]; }
        pose::offset_parts(offsets + 16 * o, ot, oz);
        pose::accumulate_row(acc, dp, dd, ot, oz);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)                    // fixed butterfly over the wave
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] += __shfl_xor(acc[i], s, 64);
    if (lane != 0) return;
    const int rd = pose::rot_dim(rep);
    float r[6], dt[3], drot[6];
    for (int i = 0; i < rd; ++i) r[i] = rot[(long)p * rd + i];
    pose::pose_vjp(rep, r, acc, scale, dt, drot);
    for (int i = 0; i < 3; ++i) d_t[(long)p * 3 + i] = dt[i];
    for (int i = 0; i < rd; ++i) d_rot[(long)p * rd + i] = drot[i];
}

__global__ void pose_adam_step_kernel(pose::AdamConfig c, int rep, int P, const int* __restrict__ train_flags, int* __restrict__ counters,
                                      const float* __restrict__ g_t, const float* __restrict__ g_rot, float* __restrict__ m_t,
                                      float* __restrict__ v_t, float* __restrict__ m_r, float* __restrict__ v_r, float* __restrict__ t,
                                      float* __restrict__ rot) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int rd = pose::rot_dim(rep);
    const int flags[2] = {train_flags[0], train_flags[1]};
    const long o3 = (long)p * 3, orr = (long)p * rd;
    float tt[3], mt[3], vt[3], gt[3], rr[6], mr[6], vr[6], gr[6];
    for (int i = 0; i < 3; ++i) { tt[i] = t[o3 + i]; mt[i] = m_t[o3 + i]; vt[i] = v_t[o3 + i]; gt[i] = g_t[o3 + i]; }
    for (int i = 0; i < rd; ++i) { rr[i] = rot[orr + i]; mr[i] = m_r[orr + i]; vr[i] = v_r[orr + i]; gr[i] = g_rot[orr + i]; }
    int ct = counters[p], cr = counters[P + p];
    pose::adam_step_pose(rep, c, flags, &ct, &cr, gt, gr, mt, vt, mr, vr, tt, rr);
    counters[p] = ct;
    counters[P + p] = cr;
    for (int i = 0; i < 3; ++i) { t[o3 + i] = tt[i]; m_t[o3 + i] = mt[i]; v_t[o3 + i] = vt[i]; }
    for (int i = 0; i < rd; ++i) { rot[orr + i] = rr[i]; m_r[orr + i] = mr[i]; v_r[orr + i] = vr[i]; }
}

}  // namespace

}  // namespace mvnerf

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------
extern "C" {

using mvnerf::aligned4;
using mvnerf::hip_status;

int mvnerf_pose_query_points(const float* t, const float* rot, int rep, const float* offsets, int P, int n5, int B, long ld, float* points,
                             float* dirs, mvnerf_stream_t stream) {
    if (!t || !rot || !offsets || !points || !dirs) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_pose_query_points: null pointer");
    if (P <= 0 || n5 <= 0 || B <= 0) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_pose_query_points: P=%d n5=%d B=%d", P, n5, B);
    if (rep != 0 && rep != 1) return mvnerf::api_fail(MVNERF_E_SHAPE, "mvnerf_pose_query_points: rep=%d (0 quaternion, 1 6d)", rep);
    if (ld < (long)P * n5) return mvnerf::api_fail(MVNERF_E_SHAPE, "mvnerf_pose_query_points: ld=%ld < P*n5=%ld", ld, (long)P * n5);
    if (!aligned4(t) || !aligned4(rot) || !aligned4(offsets) || !aligned4(points) || !aligned4(dirs))
        return mvnerf::api_fail(MVNERF_E_ALIGN, "mvnerf_pose_query_points: buffers must be 4-byte aligned");
    const long n = (long)P * n5;
    hipLaunchKernelGGL(mvnerf::pose_query_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       t, rot, rep, offsets, P, n5, B, ld, points, dirs);
    return hip_status(hipGetLastError(), "mvnerf_pose_query_points");
}

int mvnerf_pose_query_vjp(const float* rot, int rep, const float* offsets, const float* d_points, const float* d_dirs, int P, int n5, int B,
                          long ld, float scale, float* d_t, float* d_rot, mvnerf_stream_t stream) {
    if (!rot || !offsets || !d_points || !d_dirs || !d_t || !d_rot) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_pose_query_vjp: null pointer");
    if (P <= 0 || n5 <= 0 || B <= 0) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_pose_query_vjp: P=%d n5=%d B=%d", P, n5, B);
    if (rep != 0 && rep != 1) return mvnerf::api_fail(MVNERF_E_SHAPE, "mvnerf_pose_query_vjp: rep=%d (0 quaternion, 1 6d)", rep);
    if (ld < (long)P * n5) return mvnerf::api_fail(MVNERF_E_SHAPE, "mvnerf_pose_query_vjp: ld=%ld < P*n5=%ld", ld, (long)P * n5);
    if (!aligned4(rot) || !aligned4(offsets) || !aligned4(d_points) || !aligned4(d_dirs) || !aligned4(d_t) || !aligned4(d_rot))
        return mvnerf::api_fail(MVNERF_E_ALIGN, "mvnerf_pose_query_vjp: buffers must be 4-byte aligned");
    const int waves = mvnerf::kVjpWaves;
    hipLaunchKernelGGL(mvnerf::pose_query_vjp_kernel, dim3((unsigned)((P + waves - 1) / waves)), dim3(64 * waves), 0,
                       static_cast<hipStream_t>(stream), rot, rep, offsets, d_points, d_dirs, P, n5, B, ld, scale, d_t, d_rot);
    return hip_status(hipGetLastError(), "mvnerf_pose_query_vjp");
}

int mvnerf_pose_query_jvp(const float* rot, int rep, const float* offsets, const float* c_t, const float* c_rot, int P, int n5, int B, long ld,
                          float* t_points, float* t_dirs, mvnerf_stream_t stream) {
    if (!rot || !offsets || !c_t || !c_rot || !t_points || !t_dirs) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_pose_query_jvp: null pointer");
    if (P <= 0 || n5 <= 0 || B <= 0) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_pose_query_jvp: P=%d n5=%d B=%d", P, n5, B);
    if (rep != 0 && rep != 1) return mvnerf::api_fail(MVNERF_E_SHAPE, "mvnerf_pose_query_jvp: rep=%d (0 quaternion, 1 6d)", rep);
    if (ld < (long)P * n5) return mvnerf::api_fail(MVNERF_E_SHAPE, "mvnerf_pose_query_jvp: ld=%ld < P*n5=%ld", ld, (long)P * n5);
    if (!aligned4(rot) || !aligned4(offsets) || !aligned4(c_t) || !aligned4(c_rot) || !aligned4(t_points) || !aligned4(t_dirs))
        return mvnerf::api_fail(MVNERF_E_ALIGN, "mvnerf_pose_query_jvp: buffers must be 4-byte aligned");
    const long n = (long)P * n5;
    hipLaunchKernelGGL(mvnerf::pose_query_jvp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), rot, rep,
                       offsets, c_t, c_rot, P, n5, B, ld, t_points, t_dirs);
    return hip_status(hipGetLastError(), "mvnerf_pose_query_jvp");
}

int mvnerf_pose_adam_step(const mvnerf_pose_adam_config* cfg, int rep, int P, const int* train_flags, int* counters, const float* g_t,
                          const float* g_rot, float* m_t, float* v_t, float* m_r, float* v_r, float* t, float* rot, mvnerf_stream_t stream) {
    if (!cfg || !train_flags || !counters || !g_t || !g_rot || !m_t || !v_t || !m_r || !v_r || !t || !rot)
        return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_pose_adam_step: null pointer");
    if (P <= 0) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_pose_adam_step: P=%d", P);
    if (rep != 0 && rep != 1) return mvnerf::api_fail(MVNERF_E_SHAPE, "mvnerf_pose_adam_step: rep=%d (0 quaternion, 1 6d)", rep);
    if (!aligned4(train_flags) || !aligned4(counters) || !aligned4(g_t) || !aligned4(g_rot) || !aligned4(m_t) || !aligned4(v_t) || !aligned4(m_r) ||
        !aligned4(v_r) || !aligned4(t) || !aligned4(rot))
        return mvnerf::api_fail(MVNERF_E_ALIGN, "mvnerf_pose_adam_step: buffers must be 4-byte aligned");
    mvnerf::pose::AdamConfig c;
    for (int v = 0; v < 2; ++v) { c.lr0[v] = cfg->lr0[v]; c.decay[v] = cfg->decay[v]; }
    c.beta1 = cfg->beta1; c.beta2 = cfg->beta2; c.eps = cfg->eps; c.clip = cfg->clip;
    c.clip_translation = cfg->clip_translation;
    for (int i = 0; i < 3; ++i) { c.lo[i] = cfg->lo[i]; c.hi[i] = cfg->hi[i]; }
    hipLaunchKernelGGL(mvnerf::pose_adam_step_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), c,
                       rep, P, train_flags, counters, g_t, g_rot, m_t, v_t, m_r, v_r, t, rot);
    return hip_status(hipGetLastError(), "mvnerf_pose_adam_step");
}

}  // extern "C"
