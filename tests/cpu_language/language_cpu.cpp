// extern "C" shims over mvnerf_pose.h (the pose JVP) and mvnerf_language.h (the losses) so tests/test_language_math_cpu.py can call the
// per-row code on the host, with the loops and factors of the kernels (pose_ops.hip, language_ops.hip) around it.
// `wrong` != 0 selects a deliberately wrong term (the tests show that their bars catch each):
//   ml_pose_jvp   1: the 6d form without the normalisation's projection (dr = da / |a|);  2: the quaternion's w cross terms with the wrong sign
//   ml_cosine     1: the cotangent without its projection (u(l) / |x|)
//   ml_landscape  1: kl_divergence without the softmax Jacobian (d loss / d s handed on as d loss / d y)
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_language.h"
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_pose.h"

using namespace mvnerf::pose;
using namespace mvnerf::language;

static void wrong_rotation_jvp(int rep, const float* rot, const float* c_rot, float* dR, int wrong) {
    rotation_jvp(rep, rot, c_rot, dR);
    if (rep == kRepQuaternion && wrong == 2) {
        const float pairs[3][2] = {{1, 3}, {2, 6}, {5, 7}};          // R_ik and R_ki differ by the sign of their w term
        for (auto& pr : pairs) { const float a = dR[(int)pr[0]]; dR[(int)pr[0]] = dR[(int)pr[1]]; dR[(int)pr[1]] = a; }
    }
    if (rep == kRep6d && wrong == 1) {
        float r[6], d[6];
        for (int h = 0; h < 2; ++h) {
            const float* a = rot + 3 * h;
            const float n = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
            for (int i = 0; i < 3; ++i) { r[3 * h + i] = a[i] / n; d[3 * h + i] = c_rot[3 * h + i] / n; }
        }
        const float* r1 = r; const float* r2 = r + 3; const float* d1 = d; const float* d2 = d + 3;
        const float d3[3] = {(d1[1] * r2[2] - d1[2] * r2[1]) + (r1[1] * d2[2] - r1[2] * d2[1]),
                             (d1[2] * r2[0] - d1[0] * r2[2]) + (r1[2] * d2[0] - r1[0] * d2[2]),
                             (d1[0] * r2[1] - d1[1] * r2[0]) + (r1[0] * d2[1] - r1[1] * d2[0])};
        for (int i = 0; i < 3; ++i) { dR[3 * i] = d1[i]; dR[3 * i + 1] = d2[i]; dR[3 * i + 2] = d3[i]; }
    }
}

extern "C" {
// rot (P,4|6), offsets (n5,4,4), c_t (P,3), c_rot (P,4|6) -> t_points, t_dirs (P*n5, 3) in the order (pose, offset)
void ml_pose_jvp(const float* rot, int rep, const float* offsets, const float* c_t, const float* c_rot, int P, int n5, float* t_points,
                 float* t_dirs, int wrong) {
    const int rd = rot_dim(rep);
    for (int p = 0; p < P; ++p) {
        float dR[9];
        wrong_rotation_jvp(rep, rot + rd * p, c_rot + rd * p, dR, wrong);
        for (int o = 0; o < n5; ++o) {
            float ot[3], oz[3];
            offset_parts(offsets + 16 * o, ot, oz);
            const long row = (long)p * n5 + o;
            query_point_jvp(dR, c_t + 3 * p, ot, oz, t_points + 3 * row, t_dirs + 3 * row);
        }
    }
}

// landscape_loss_kernel: y, label (B, np) -> loss[0] = mean over the batch, g_y = weight * d total / d y
void ml_landscape(const float* y, const float* label, int B, int np, int kind, float weight, float* g_y, float* loss, int wrong) {
    const float coef = kind == kLossCrossEntropy ? weight / (float)B : weight;
    float total = 0.0f;
    for (int b = 0; b < B; ++b) {
        float* g = g_y + (long)b * np;
        total += landscape_row(kind, y + (long)b * np, label + (long)b * np, np, g);
        if (wrong == 1 && kind == kLossKL) {
            const float* yb = y + (long)b * np;
            float m = yb[0], z = 0.0f;
            for (int j = 1; j < np; ++j) m = fmaxf(m, yb[j]);
            for (int j = 0; j < np; ++j) z += expf(yb[j] - m);
            for (int j = 0; j < np; ++j) g[j] = -(clip01(label[(long)b * np + j]) / clip01(expf(yb[j] - m) / z));
        }
        for (int j = 0; j < np; ++j) g[j] = coef * g[j];
    }
    loss[0] = total / (float)B;
}

// cosine_loss_kernel: x, label (rows, dim), dim 6 = two halves of 3 -> loss[0] = -mean, g_x = scale * d loss / d x
void ml_cosine(const float* x, const float* label, long rows, int dim, float scale, float* g_x, float* loss, int wrong) {
    const int halves = dim == 6 ? 2 : 1, d = dim == 6 ? 3 : dim;
    const float coef = -(scale / (float)rows);
    float total = 0.0f;
    for (long r = 0; r < rows; ++r)
        for (int h = 0; h < halves; ++h) {
            const long at = r * dim + 3 * h;
            float g[4];
            total += cosine_row(x + at, label + at, d, g);
            if (wrong == 1) {
                float ssx = 0.0f, ssl = 0.0f;
                for (int i = 0; i < d; ++i) { ssx += x[at + i] * x[at + i]; ssl += label[at + i] * label[at + i]; }
                for (int i = 0; i < d; ++i) g[i] = (label[at + i] / sqrtf(fmaxf(ssl, kCosClamp))) / sqrtf(fmaxf(ssx, kCosClamp));
            }
            for (int i = 0; i < d; ++i) g_x[at + i] = coef * g[i];
        }
    loss[0] = -(total / (float)rows);
}
}
