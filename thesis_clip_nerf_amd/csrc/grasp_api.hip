// extern "C" grasp-pose optimisation step: DNGFOptimizer.optimize_pose (lmvnerf/grasp_optimizer.py:158-184) through a frozen LanguageNeRF
// (lmvnerf/model_v4.py:208-265) behind ONE call, so that a host in any language can move grasp poses uphill without re-implementing the
// sequencing thesis_clip_nerf_amd/grasp_optimizer.py does in Python:
//   mvnerf_grasp_success               = poses -> query points -> trunk -> head -> per-pose tail                     (stages 1-4)
//   mvnerf_grasp_success_and_gradients = the same with stashes, then tail VJP -> head VJP -> trunk VJP -> pose VJP  (stages 1-7)
//   mvnerf_grasp_opt_step              = the above and clip + Keras Adam + post_process                             (stages 1-8)
// No allocation: every intermediate lives in the caller's workspace (mvnerf_grasp_workspace_bytes).  Stream-ordered, no host
// synchronisation, no global state.
#include <hip/hip_runtime.h>

#include "../../include/mvnerf_hip.h"
#include "mvnerf_kernels.h"

namespace {

constexpr size_t kAlign = 256;
size_t up(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

struct GraspWs {
    float *points, *dirs, *z, *rgbs, *acts, *c, *y, *tail_stash, *g_x, *g_acts, *d_points, *d_dirs;
    void *field_ws, *vjp_scratch;
    float* stash;
    long n, ld;           // rows of one scene: P * n5, and padded to whole 32-point tiles when V > 1
    size_t bytes;
};

GraspWs carve_grasp(void* base, int B, int V, int P, int n5) {
    GraspWs w;
    char* p = static_cast<char*>(base);
    auto take = [&](size_t bytes) {
        char* q = p;
        p += up(bytes);
        return q;
    };
    w.n = (long)P * n5;
    w.ld = V > 1 ? (w.n + 31) / 32 * 32 : w.n;
    const size_t rows = (size_t)B * w.ld;
    w.points = reinterpret_cast<float*>(take(rows * 3 * 4));
    w.dirs = reinterpret_cast<float*>(take(rows * 3 * 4));
    w.z = reinterpret_cast<float*>(take(rows * 4));
    w.rgbs = reinterpret_cast<float*>(take(rows * 4 * 4));
    w.field_ws = take(mvnerf_field_workspace_bytes(B, V, (int)w.ld));
    w.stash = reinterpret_cast<float*>(take(mvnerf_stash_bytes(B, V, (int)w.ld, 1)));
    w.acts = reinterpret_cast<float*>(take(rows * 4 * 128 * 4));
    w.c = reinterpret_cast<float*>(take(rows * 256 * 4));
    w.y = reinterpret_cast<float*>(take(rows * 64 * 4));
    w.tail_stash = reinterpret_cast<float*>(take((size_t)B * P * mvnerf::grasp_tail_stash_floats() * 4));
    w.g_x = reinterpret_cast<float*>(take(rows * 64 * 4));
    w.g_acts = reinterpret_cast<float*>(take(rows * 4 * 128 * 4));
    w.vjp_scratch = take(mvnerf_query_vjp_scratch_bytes(B, V, (int)w.ld));
    w.d_points = reinterpret_cast<float*>(take(rows * 3 * 4));
    w.d_dirs = reinterpret_cast<float*>(take(rows * 3 * 4));
    w.bytes = (size_t)(p - static_cast<char*>(base));
    return w;
}

bool sizes_ok(int B, int V, int P, int n5) {
    return B > 0 && V > 0 && P > 0 && n5 > 0 && n5 <= 4096 && (long)P * n5 + 31 < (1L << 31) / B;
}

// rows n .. ld of every scene repeat row n - 1 (whole tiles for the multi-view kernels; their cotangents stay zero)
__global__ void pad_rows_kernel(float* __restrict__ points, float* __restrict__ dirs, int B, long n, long ld) {
    const long pad = ld - n, idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * pad * 3) return;
    const long b = idx / (pad * 3), r = (idx / 3) % pad;
    const int k = (int)(idx % 3);
    points[(b * ld + n + r) * 3 + k] = points[(b * ld + n - 1) * 3 + k];
    dirs[(b * ld + n + r) * 3 + k] = dirs[(b * ld + n - 1) * 3 + k];
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

#define MV_RC(x)                  \
    do {                          \
        int rc_ = (x);            \
        if (rc_ != 0) return rc_; \
    } while (0)
#define MV_HIP(x, who)                                                                                    \
    do {                                                                                                  \
        hipError_t e_ = (x);                                                                              \
        if (e_ != hipSuccess) return mvnerf::api_fail((int)e_, "%s: %s", who, hipGetErrorString(e_));     \
    } while (0)

int validate(const mvnerf_grasp_call* c, bool want_grads, const char* who, GraspWs* out) {
    using mvnerf::api_fail;
    if (!c) return api_fail(MVNERF_E_ARG, "%s: null call", who);
    if (!c->images || !c->features || !c->intrinsics || !c->extrinsics_inv || !c->packed_net || !c->split || !c->bwd_streams || !c->head_packed ||
        !c->head_b4 || !c->head_bc || !c->tail_packed || !c->offsets || !c->t || !c->rot || !c->success || !c->workspace)
        return api_fail(MVNERF_E_ARG, "%s: null pointer", who);
    if (want_grads && (!c->g_t || !c->g_rot)) return api_fail(MVNERF_E_ARG, "%s: null pointer (g_t, g_rot)", who);
    if (!sizes_ok(c->B, c->V, c->P, c->n5) || c->H < 2 || c->W < 2)
        return api_fail(MVNERF_E_ARG, "%s: B=%d V=%d H=%d W=%d P=%d n5=%d", who, c->B, c->V, c->H, c->W, c->P, c->n5);
    if (c->rep != 0 && c->rep != 1) return api_fail(MVNERF_E_SHAPE, "%s: rep=%d (0 quaternion, 1 6d)", who, c->rep);
    if (!al16(c->features) || !al16(c->packed_net) || !al16(c->split) || !al16(c->bwd_streams) || !al16(c->head_packed) || !al16(c->tail_packed))
        return api_fail(MVNERF_E_ALIGN, "%s: features, packed_net, split, bwd_streams, head_packed, tail_packed must be 16-byte aligned", who);
    if (!al4(c->images) || !al4(c->intrinsics) || !al4(c->extrinsics_inv) || !al4(c->head_b4) || !al4(c->head_bc) || !al4(c->offsets) ||
        !al4(c->t) || !al4(c->rot) || !al4(c->success) || !al4(c->g_t) || !al4(c->g_rot))
        return api_fail(MVNERF_E_ALIGN, "%s: float buffers must be 4-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(c->workspace) & 255u) != 0) return api_fail(MVNERF_E_ALIGN, "%s: workspace must be 256-byte aligned", who);
    *out = carve_grasp(c->workspace, c->B, c->V, c->P, c->n5);
    if (c->workspace_bytes < out->bytes)
        return api_fail(MVNERF_E_ARG, "%s: workspace %zu bytes, need %zu (mvnerf_grasp_workspace_bytes)", who, c->workspace_bytes, out->bytes);
    return 0;
}

// stages 1-4 (and 5-7 when want_grads)
int run(const mvnerf_grasp_call* c, bool want_grads, const char* who, mvnerf_stream_t stream) {
    GraspWs w;
    MV_RC(validate(c, want_grads, who, &w));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = c->B, V = c->V, P = c->P, n5 = c->n5, ld = (int)w.ld;
    const long rows = (long)B * w.ld;
    const bool padded = w.ld > w.n;
    const size_t tail_stash = mvnerf::grasp_tail_stash_floats();
    // 1. poses -> query points
    MV_RC(mvnerf_pose_query_points(c->t, c->rot, c->rep, c->offsets, P, n5, B, w.ld, w.points, w.dirs, stream));
    if (padded) {
        const long n_pad = (long)B * (w.ld - w.n) * 3;
        hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, st, w.points, w.dirs, B, w.n, w.ld);
        MV_HIP(hipGetLastError(), who);
    }
    // 2. the frozen trunk, pre-activations kept; its four fused activations as rows
    MV_HIP(mvnerf::launch_zero(w.z, (size_t)rows * 4, st), who);
    MV_RC(mvnerf_field_eval_stash_split(w.points, w.dirs, w.z, c->images, c->features, nullptr, c->intrinsics, c->extrinsics_inv, c->packed_net,
                                        c->split, B, V, ld, 1, c->H, c->W, w.rgbs, w.stash, w.field_ws, stream));
    MV_RC(mvnerf_stash_fused_acts(w.stash, B, V, ld, w.acts, stream));
    // 3. the per-point read-out (pad rows included: they are whole rows of the same tensors)
    MV_RC(mvnerf_grasp_head_fwd(w.acts, c->head_packed, c->head_b4, c->head_bc, rows, w.c, w.y, stream));
    // 4. the per-pose read-out: a scene's P rows of n5 * 64 lie side by side in y; padded scenes are ld * 64 floats apart
    const int calls = padded ? B : 1;
    const long m_call = padded ? P : (long)B * P;
    for (int b = 0; b < calls; ++b)
        MV_RC(mvnerf_grasp_tail_fwd(w.y + (size_t)b * w.ld * 64, c->tail_packed, m_call, n5, c->success + (size_t)b * P,
                                    want_grads ? w.tail_stash + (size_t)b * P * tail_stash : nullptr, stream));
    if (!want_grads) return 0;
    // 4'. d(sum success) / dx, pad rows zero
    if (padded)
        for (int b = 0; b < B; ++b) MV_HIP(mvnerf::launch_zero(w.g_x + ((size_t)b * w.ld + w.n) * 64, (size_t)(w.ld - w.n) * 64 * 4, st), who);
    for (int b = 0; b < calls; ++b)
        MV_RC(mvnerf_grasp_tail_vjp(w.y + (size_t)b * w.ld * 64, nullptr, w.tail_stash + (size_t)b * P * tail_stash, c->tail_packed, m_call, n5,
                                    w.g_x + (size_t)b * w.ld * 64, stream));
    // 5.-7. head VJP -> trunk VJP -> pose VJP of loss = -sum success
    MV_RC(mvnerf_grasp_head_vjp_acts(w.g_x, w.c, w.y, c->head_packed, rows, w.g_acts, stream));
    MV_RC(mvnerf_query_vjp(w.points, w.dirs, c->images, c->features, c->intrinsics, c->extrinsics_inv, c->bwd_streams, w.stash, w.g_acts, B, V, ld,
                           c->H, c->W, w.vjp_scratch, w.d_points, w.d_dirs, stream));
    MV_RC(mvnerf_pose_query_vjp(c->rot, c->rep, c->offsets, w.d_points, w.d_dirs, P, n5, B, w.ld, -1.0f, c->g_t, c->g_rot, stream));
    return 0;
}

}  // namespace

extern "C" {

size_t mvnerf_grasp_workspace_bytes(int B, int V, int P, int n5) {
    if (!sizes_ok(B, V, P, n5)) return 0;
    return carve_grasp(nullptr, B, V, P, n5).bytes;
}

int mvnerf_grasp_success(const mvnerf_grasp_call* call, mvnerf_stream_t stream) { return run(call, false, "mvnerf_grasp_success", stream); }

int mvnerf_grasp_success_and_gradients(const mvnerf_grasp_call* call, mvnerf_stream_t stream) {
    return run(call, true, "mvnerf_grasp_success_and_gradients", stream);
}

int mvnerf_grasp_opt_step(const mvnerf_grasp_call* call, const mvnerf_pose_adam_config* cfg, const int* train_flags, int* counters, float* m_t,
                          float* v_t, float* m_r, float* v_r, mvnerf_stream_t stream) {
    if (!cfg || !train_flags || !counters || !m_t || !v_t || !m_r || !v_r)
        return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_opt_step: null pointer (cfg, train_flags, counters, moments)");
    MV_RC(run(call, true, "mvnerf_grasp_opt_step", stream));
    return mvnerf_pose_adam_step(cfg, call->rep, call->P, train_flags, counters, call->g_t, call->g_rot, m_t, v_t, m_r, v_r, call->t, call->rot,
                                 stream);
}

}  // extern "C"
