// extern "C" grasp-pose optimisation step: DNGFOptimizer.optimize_pose (lmvnerf/grasp_optimizer.py:158-184) through a frozen LanguageNeRF
// (lmvnerf/model_v4.py:208-265) behind ONE call, so that a host in any language can move grasp poses uphill without re-implementing the
// sequencing thesis_clip_nerf_amd/grasp_optimizer.py does in Python:
//   mvnerf_grasp_success               = poses -> query points -> trunk -> head -> per-pose tail                     (stages 1-4)
//   mvnerf_grasp_success_and_gradients = the same with stashes, then tail VJP -> head VJP -> trunk VJP -> pose VJP  (stages 1-7)
//   mvnerf_grasp_opt_step              = the above and clip + Keras Adam + post_process                             (stages 1-8)
// No allocation: every intermediate lives in the caller's workspace (mvnerf_grasp_workspace_bytes).  Stream-ordered, no host
// synchronisation, no global state.
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"

namespace {

using mvnerf::aligned16;
using mvnerf::aligned4;

struct GraspWs {
    float *points, *dirs, *z, *rgbs, *acts, *c, *y, *tail_stash, *g_x, *g_acts, *d_points, *d_dirs;
    void *field_ws, *vjp_scratch;
    float* stash;
    long n, ld;           // rows of one scene: P * n5, and padded to whole 32-point tiles when V > 1
    size_t bytes;
};

// bf16: the trunk runs as mvnerf_query_stash_bf16 / mvnerf_query_vjp_bf16 - relu bits in the stash's place, their workspace and scratch
GraspWs carve_grasp(void* base, int B, int V, int P, int n5, bool bf16 = false) {
    GraspWs w;
    mvnerf::Bump ws(base);
    w.n = (long)P * n5;
    w.ld = mvnerf::pose_rows_ld(V, w.n);
    const size_t rows = (size_t)B * w.ld;
    w.points = ws.floats(rows * 3);
    w.dirs = ws.floats(rows * 3);
    w.z = ws.floats(rows);
    w.rgbs = ws.floats(rows * 4);
    w.field_ws = ws.take(bf16 ? mvnerf_query_workspace_bytes(B, V, (int)w.ld) : mvnerf_field_workspace_bytes(B, V, (int)w.ld));
    w.stash = static_cast<float*>(ws.take(bf16 ? mvnerf_relu_bits_bytes(B, V, (int)w.ld) : mvnerf_stash_bytes(B, V, (int)w.ld, 1)));
    w.acts = ws.floats(rows * 4 * 128);
    w.c = ws.floats(rows * 256);
    w.y = ws.floats(rows * 64);
    w.tail_stash = ws.floats((size_t)B * P * mvnerf::grasp_tail_stash_floats());
    w.g_x = ws.floats(rows * 64);
    w.g_acts = ws.floats(rows * 4 * 128);
    w.vjp_scratch = ws.take(bf16 ? mvnerf_query_vjp_bf16_scratch_bytes(B, V, (int)w.ld) : mvnerf_query_vjp_scratch_bytes(B, V, (int)w.ld));
    w.d_points = ws.floats(rows * 3);
    w.d_dirs = ws.floats(rows * 3);
    w.bytes = ws.bytes();
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

// The trunk's bf16 operands of the _bf16 entry points; both NULL: the fp32-grade path
struct Bf16Nets {
    const void *packed16, *bwd16;
};

int validate(const mvnerf_grasp_call* c, bool want_grads, const char* who, GraspWs* out, const Bf16Nets* bf16) {
    using mvnerf::api_fail;
    if (!c) return api_fail(MVNERF_E_ARG, "%s: null call", who);
    if (bf16 && (!bf16->packed16 || !bf16->bwd16)) return api_fail(MVNERF_E_ARG, "%s: null pointer (packed16, bwd16)", who);
    if (!c->images || !c->features || !c->intrinsics || !c->extrinsics_inv || !c->packed_net || (!bf16 && !c->split) || !c->bwd_streams || !c->head_packed ||
        !c->head_b4 || !c->head_bc || !c->tail_packed || !c->offsets || !c->t || !c->rot || !c->success || !c->workspace)
        return api_fail(MVNERF_E_ARG, "%s: null pointer", who);
    if (want_grads && (!c->g_t || !c->g_rot)) return api_fail(MVNERF_E_ARG, "%s: null pointer (g_t, g_rot)", who);
    if (!sizes_ok(c->B, c->V, c->P, c->n5) || c->H < 2 || c->W < 2)
        return api_fail(MVNERF_E_ARG, "%s: B=%d V=%d H=%d W=%d P=%d n5=%d", who, c->B, c->V, c->H, c->W, c->P, c->n5);
    if (c->rep != 0 && c->rep != 1) return api_fail(MVNERF_E_SHAPE, "%s: rep=%d (0 quaternion, 1 6d)", who, c->rep);
    if (!aligned16(c->features) || !aligned16(c->packed_net) || !aligned16(c->split) || !aligned16(c->bwd_streams) ||
        !aligned16(c->head_packed) || !aligned16(c->tail_packed))
        return api_fail(MVNERF_E_ALIGN, "%s: features, packed_net, split, bwd_streams, head_packed, tail_packed must be 16-byte aligned", who);
    if (bf16 && (!aligned16(bf16->packed16) || !aligned16(bf16->bwd16))) return api_fail(MVNERF_E_ALIGN, "%s: packed16, bwd16 must be 16-byte aligned", who);
    if (!aligned4(c->images) || !aligned4(c->intrinsics) || !aligned4(c->extrinsics_inv) || !aligned4(c->head_b4) || !aligned4(c->head_bc) ||
        !aligned4(c->offsets) || !aligned4(c->t) || !aligned4(c->rot) || !aligned4(c->success) || !aligned4(c->g_t) || !aligned4(c->g_rot))
        return api_fail(MVNERF_E_ALIGN, "%s: float buffers must be 4-byte aligned", who);
    if (!mvnerf::aligned256(c->workspace)) return api_fail(MVNERF_E_ALIGN, "%s: workspace must be 256-byte aligned", who);
    *out = carve_grasp(c->workspace, c->B, c->V, c->P, c->n5, bf16 != nullptr);
    if (c->workspace_bytes < out->bytes)
        return api_fail(MVNERF_E_ARG, "%s: workspace %zu bytes, need %zu (mvnerf_grasp_workspace_bytes%s)", who, c->workspace_bytes, out->bytes,
                        bf16 ? "_bf16" : "");
    return 0;
}

// stages 1-4 (and 5-7 when want_grads)
int run(const mvnerf_grasp_call* c, bool want_grads, const char* who, mvnerf_stream_t stream, const Bf16Nets* bf16 = nullptr) {
    GraspWs w;
    MV_RC(validate(c, want_grads, who, &w, bf16));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = c->B, V = c->V, P = c->P, n5 = c->n5, ld = (int)w.ld;
    const long rows = (long)B * w.ld;
    const bool padded = w.ld > w.n;
    const size_t tail_stash = mvnerf::grasp_tail_stash_floats();
    // 1. poses -> query points
    MV_RC(mvnerf_pose_query_points(c->t, c->rot, c->rep, c->offsets, P, n5, B, w.ld, w.points, w.dirs, stream));
    MV_RC(mvnerf::pad_pose_rows(who, w.points, w.dirs, B, w.n, w.ld, st));
    // 2. the frozen trunk, pre-activations kept; its four fused activations as rows
    if (bf16) {
        MV_RC(mvnerf_query_stash_bf16(w.points, w.dirs, c->images, c->features, c->intrinsics, c->extrinsics_inv, c->packed_net, bf16->packed16, B,
                                      V, ld, c->H, c->W, w.acts, w.stash, w.field_ws, stream));
    } else {
        MV_HIP(mvnerf::launch_zero(w.z, (size_t)rows * 4, st), who);
        MV_RC(mvnerf::pose_rows_trunk(w.points, w.dirs, w.z, c->images, c->features, c->intrinsics, c->extrinsics_inv, c->packed_net, c->split, B,
                                      V, w.ld, c->H, c->W, w.rgbs, w.stash, w.field_ws, w.acts, stream));
    }
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
    if (bf16)
        MV_RC(mvnerf_query_vjp_bf16(w.points, w.dirs, c->images, c->features, c->intrinsics, c->extrinsics_inv, c->bwd_streams, bf16->bwd16, w.stash,
                                    w.g_acts, B, V, ld, c->H, c->W, w.vjp_scratch, w.d_points, w.d_dirs, stream));
    else
        MV_RC(mvnerf_query_vjp(w.points, w.dirs, c->images, c->features, c->intrinsics, c->extrinsics_inv, c->bwd_streams, w.stash, w.g_acts, B, V,
                               ld, c->H, c->W, w.vjp_scratch, w.d_points, w.d_dirs, stream));
    MV_RC(mvnerf_pose_query_vjp(c->rot, c->rep, c->offsets, w.d_points, w.d_dirs, P, n5, B, w.ld, -1.0f, c->g_t, c->g_rot, stream));
    return 0;
}

}  // namespace

int mvnerf::pad_pose_rows(const char* who, float* points, float* dirs, int B, long n, long ld, hipStream_t st) {
    if (ld == n) return 0;
    const long n_pad = (long)B * (ld - n) * 3;
    hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, st, points, dirs, B, n, ld);
    return hip_status(hipGetLastError(), who);
}

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

size_t mvnerf_grasp_workspace_bytes_bf16(int B, int V, int P, int n5) {
    if (!sizes_ok(B, V, P, n5)) return 0;
    return carve_grasp(nullptr, B, V, P, n5, true).bytes;
}

int mvnerf_grasp_success_bf16(const mvnerf_grasp_call* call, const void* packed16, const void* bwd16, mvnerf_stream_t stream) {
    const Bf16Nets nets = {packed16, bwd16};
    return run(call, false, "mvnerf_grasp_success_bf16", stream, &nets);
}

int mvnerf_grasp_success_and_gradients_bf16(const mvnerf_grasp_call* call, const void* packed16, const void* bwd16, mvnerf_stream_t stream) {
    const Bf16Nets nets = {packed16, bwd16};
    return run(call, true, "mvnerf_grasp_success_and_gradients_bf16", stream, &nets);
}

int mvnerf_grasp_opt_step_bf16(const mvnerf_grasp_call* call, const void* packed16, const void* bwd16, const mvnerf_pose_adam_config* cfg,
                               const int* train_flags, int* counters, float* m_t, float* v_t, float* m_r, float* v_r, mvnerf_stream_t stream) {
    if (!cfg || !train_flags || !counters || !m_t || !v_t || !m_r || !v_r)
        return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_grasp_opt_step_bf16: null pointer (cfg, train_flags, counters, moments)");
    const Bf16Nets nets = {packed16, bwd16};
    MV_RC(run(call, true, "mvnerf_grasp_opt_step_bf16", stream, &nets));
    return mvnerf_pose_adam_step(cfg, call->rep, call->P, train_flags, counters, call->g_t, call->g_rot, m_t, v_t, m_r, v_r, call->t, call->rot,
                                 stream);
}

}  // extern "C"
