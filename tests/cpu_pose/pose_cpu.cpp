// extern "C" shims over mvnerf_pose.h so tests/test_pose_math_cpu.py can call the per-pose code on the host.
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_pose.h"

using namespace mvnerf::pose;

extern "C" {
// t (P,3), rot (P,4|6), offsets (n5,4,4) -> points, dirs (P*n5, 3) in the order (pose, offset)
void mp_query_points(const float* t, const float* rot, int rep, const float* offsets, int P, int n5, float* points, float* dirs) {
    const int rd = rot_dim(rep);
    for (int p = 0; p < P; ++p) {
        float R[9];
        rotation(rep, rot + rd * p, R);
        for (int o = 0; o < n5; ++o) {
            float ot[3], oz[3];
            offset_parts(offsets + 16 * o, ot, oz);
            const long row = (long)p * n5 + o;
            query_point(R, t + 3 * p, ot, oz, points + 3 * row, dirs + 3 * row);
        }
    }
}
// d_points, d_dirs (B, P*n5, 3) -> scale * (d_t (P,3), d_rot (P,4|6)); rows summed b-major, as one lane of the kernel would
void mp_query_vjp(const float* rot, int rep, const float* offsets, const float* d_points, const float* d_dirs, int P, int n5, int B,
                  float scale, float* d_t, float* d_rot) {
    const int rd = rot_dim(rep);
    for (int p = 0; p < P; ++p) {
        float acc[12] = {0};
        for (int b = 0; b < B; ++b)
            for (int o = 0; o < n5; ++o) {
                float ot[3], oz[3];
                offset_parts(offsets + 16 * o, ot, oz);
                const long row = (long)b * P * n5 + (long)p * n5 + o;
                accumulate_row(acc, d_points + 3 * row, d_dirs + 3 * row, ot, oz);
            }
        pose_vjp(rep, rot + rd * p, acc, scale, d_t + 3 * p, d_rot + rd * p);
    }
}
// one step of every pose (pose_adam_step_kernel's body); cfg: lr0[2] decay[2] beta1 beta2 eps clip lo[3] hi[3] (14 floats)
void mp_adam_step(const float* cfg, int clip_translation, int rep, int P, const int* flags, int* counters, const float* g_t,
                  const float* g_rot, float* m_t, float* v_t, float* m_r, float* v_r, float* t, float* rot) {
    AdamConfig c;
    c.lr0[0] = cfg[0]; c.lr0[1] = cfg[1]; c.decay[0] = cfg[2]; c.decay[1] = cfg[3];
    c.beta1 = cfg[4]; c.beta2 = cfg[5]; c.eps = cfg[6]; c.clip = cfg[7];
    c.clip_translation = clip_translation;
    for (int i = 0; i < 3; ++i) { c.lo[i] = cfg[8 + i]; c.hi[i] = cfg[11 + i]; }
    const int rd = rot_dim(rep);
    for (int p = 0; p < P; ++p)
        adam_step_pose(rep, c, flags, counters + p, counters + P + p, g_t + 3 * p, g_rot + rd * p, m_t + 3 * p, v_t + 3 * p, m_r + rd * p,
                       v_r + rd * p, t + 3 * p, rot + rd * p);
}
}
