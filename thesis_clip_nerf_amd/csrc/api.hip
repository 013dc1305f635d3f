// extern "C" surface of libmvnerf_hip.so (include/mvnerf_hip.h): argument validation, launch
// orchestration, error reporting.  No allocation, no host synchronisation; global state: the thread-local
// error string and the two process-wide switches mvnerf_set_split_kernel / mvnerf_set_deterministic (the
// _ex entry points choose the split kernel per call instead); safe to call from one process per GPU on any stream.
// Of several faults in one call the first in this order is reported: null pointers, sizes, int32 index
// ranges, alignment.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <atomic>

#include "mvnerf_api.h"
#include "mvnerf_math.h"
#include "mvnerf_pack.h"

namespace {
thread_local char g_err[512] = "";
}  // namespace

namespace mvnerf {
int api_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace mvnerf

namespace {

constexpr auto& fail = mvnerf::api_fail;

using mvnerf::aligned16, mvnerf::aligned4, mvnerf::hip_status, mvnerf::StashLayout;

// The two arguments the _ex entry points add: `which` (-1 or a MVNERF_SPLIT_* value) is checked before everything else, the
// alignment of `range_status` with the other alignments (after them).
int split_choice_check(const char* who, int which) {
    if (which < -1 || which > MVNERF_SPLIT_BF16X6_32)
        return fail(MVNERF_E_ARG, "%s: which=%d (-1 process-wide, 0 f16x3, 1 bf16x6, 2 bf16x6 as 32x32x16)", who, which);
    return 0;
}
int range_status_check(const char* who, const float* range_status) {
    if (!aligned4(range_status)) return fail(MVNERF_E_ALIGN, "%s: range_status must be 4-byte aligned", who);
    return 0;
}

struct Workspace {          // carve-up of the caller's scratch for mvnerf_render_fwd (floats)
    float *z, *rgbs_c, *weights, *z_all, *rgbs_f, *dir_bias;
    size_t bytes;
};

Workspace carve(void* base, long n_rays, int V, int S) {
    Workspace w;
    mvnerf::Bump ws(base, sizeof(float));           // (packed: the pieces follow each other float by float)
    const size_t n = (size_t)n_rays * S;
    w.z = ws.floats(n);
    w.weights = ws.floats(n);
    w.z_all = ws.floats(2 * n);
    w.rgbs_c = ws.floats(4 * n);
    w.rgbs_f = ws.floats(8 * n);
    w.dir_bias = ws.floats((size_t)n_rays * V * 128);
    w.bytes = ws.bytes();
    return w;
}

// ---- one field pass: the arguments of the seven mvnerf_field_eval* entry points in one shape -------------------
struct FieldArgs {
    const float *rays_o, *rays_d, *z, *images, *features, *texel_table, *intrinsics, *extrinsics_inv, *packed_net;
    const void* second;          // the bf16 / split weight stream of the kernels that read one
    int B, V, R, S, H, W;
    float* rgbs;                 // outputs an entry point does not have stay NULL
    int32_t* tap_idx;
    float *pix, *embedding, *acts_per_view, *acts_fused, *stash;
    void* workspace;
};

enum FieldKernel { kFieldFp32, kFieldBf16, kFieldBf16Maps, kFieldSplit };      // every kernel but the first reads `second`

struct FieldKind {
    FieldKernel kernel;
    bool stash;                  // training-mode pass: `stash` is required and sets its own limits
    int hw_code;                 // H < 2 or W < 2 is MVNERF_E_SHAPE, from the stash pair MVNERF_E_ARG
};

// Checks the arguments (null, sizes, index range, alignment) and fills the kernels' FieldParams; 0 or the error code.
int field_params(const char* who, const FieldArgs& a, FieldKind kind, mvnerf::FieldParams* out) {
    if (!a.rays_o || !a.rays_d || !a.z || !a.images || !a.features || !a.intrinsics || !a.extrinsics_inv || !a.packed_net || !a.rgbs ||
        !a.workspace || (kind.kernel != kFieldFp32 && !a.second) || (kind.stash && !a.stash))
        return fail(MVNERF_E_ARG, "%s: null pointer", who);
    if (a.B <= 0 || a.V <= 0 || a.R <= 0 || a.S <= 0) return fail(MVNERF_E_ARG, "%s: B=%d V=%d R=%d S=%d", who, a.B, a.V, a.R, a.S);
    if (a.H < 2 || a.W < 2) return fail(kind.hw_code, "%s: source image %dx%d, need H,W >= 2 (bilinear taps)", who, a.H, a.W);
    if (kind.stash && a.V > 1 && ((long)a.R * a.S) % 32 != 0)
        return fail(MVNERF_E_SHAPE, "%s: R*S=%ld must be a multiple of 32 when V > 1", who, (long)a.R * a.S);
    const StashLayout L(a.B, a.V, (long)a.R * a.S);
    const long total = L.total, n_tiles = L.n_tiles;
    if (total >= (1L << 31) || (long)a.B * a.V * a.H * a.W >= (1L << 31))
        return fail(MVNERF_E_SHAPE, "%s: B*R*S=%ld or B*V*H*W too large for int32 indices", who, total);
    if (kind.stash && L.view_tiles >= (1L << 18))             // stash slots are addressed with 32-bit byte offsets (16 KiB per tile)
        return fail(MVNERF_E_SHAPE, "%s: V*B*R*S/32 = %ld tiles per stash slot, at most 262143", who, L.view_tiles);
    if (!aligned16(a.features) || !aligned16(a.texel_table) || !aligned16(a.packed_net) || !aligned16(a.second) || !aligned16(a.rgbs) ||
        !aligned16(a.tap_idx) || !aligned16(a.embedding) || !aligned16(a.acts_per_view) || !aligned16(a.acts_fused) || !aligned16(a.stash) ||
        !aligned16(a.workspace))           // (NULL counts as aligned: the optional ones are checked when given)
        return fail(MVNERF_E_ALIGN, "%s: features, texel_table, packed nets, rgbs, tap_idx, embedding, acts, stash, workspace must be 16-byte aligned", who);
    mvnerf::FieldParams p = {};
    p.rays_o = a.rays_o; p.rays_d = a.rays_d; p.z = a.z; p.images = a.images; p.features = a.features;
    p.texel_table = a.texel_table;
    p.k4 = a.intrinsics; p.einv = a.extrinsics_inv; p.net = a.packed_net; p.rgbs = a.rgbs; p.tap_idx = a.tap_idx; p.pix = a.pix;
    p.embedding = a.embedding; p.acts_view = a.acts_per_view; p.acts_fused = a.acts_fused;
    p.dir_bias = static_cast<float*>(a.workspace);
    p.B = a.B; p.V = a.V; p.R = a.R; p.S = a.S; p.H = a.H; p.W = a.W;
    p.total = total;
    p.n_tiles = n_tiles;
    if (a.stash) {
        p.stash = a.stash;
        p.stash_stride = L.view_stride();
        p.stash_fused = a.stash + L.fused_slot(0);
        p.stash_fused_stride = L.fused_stride();
    }
    *out = p;
    return 0;
}

// which / range_status: the split kernel of this call and its optional range status (the _ex entry points); the others pass -1, NULL
int field_pass(const char* who, const FieldArgs& a, FieldKind kind, mvnerf_stream_t stream, int which = -1, float* range_status = nullptr) {
    if (const int rc = split_choice_check(who, which)) return rc;
    mvnerf::FieldParams p;
    if (const int rc = field_params(who, a, kind, &p)) return rc;
    if (const int rc = range_status_check(who, range_status)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (kind.kernel == kFieldFp32) return hip_status(mvnerf::launch_field_eval(p, st), who);
    if (kind.kernel == kFieldSplit) return hip_status(mvnerf::launch_field_eval_split(p, a.second, st, which, range_status), who);
    return hip_status(mvnerf::launch_field_eval_bf16(p, a.second, st, kind.kernel == kFieldBf16Maps), who);
}

// The arguments the three mvnerf_project_texels* entry points share; 0 or the error code.
int texels_check(const char* who, const void* features, const void* net, const void* net_b, int B, int V, int H, int W,
                 const float* texel_table, const float* texel_table_b) {
    if (!features || !net || !texel_table) return fail(MVNERF_E_ARG, "%s: null pointer", who);
    if ((net_b == nullptr) != (texel_table_b == nullptr)) return fail(MVNERF_E_ARG, "%s: the second net and the second table go together", who);
    if (B <= 0 || V <= 0 || H < 2 || W < 2) return fail(MVNERF_E_ARG, "%s: B=%d V=%d H=%d W=%d", who, B, V, H, W);
    if ((long)B * V * H * W >= (1L << 31)) return fail(MVNERF_E_SHAPE, "%s: B*V*H*W too large for int32 indices", who);
    if (!aligned16(features) || !aligned16(net) || !aligned16(net_b) || !aligned16(texel_table) || !aligned16(texel_table_b))
        return fail(MVNERF_E_ALIGN, "%s: features, packed nets, texel tables must be 16-byte aligned", who);
    return 0;
}

}  // namespace

extern "C" {

int mvnerf_abi_version(void) { return 1; }

const char* mvnerf_last_error(void) { return g_err; }

size_t mvnerf_packed_net_floats(void) { return (size_t)mvnerf::kPackTotal; }

int mvnerf_pack_net(const float* net_keras, float* packed, mvnerf_stream_t stream) {
    if (!net_keras || !packed) return fail(MVNERF_E_ARG, "mvnerf_pack_net: null pointer");
    if (!aligned16(packed)) return fail(MVNERF_E_ALIGN, "mvnerf_pack_net: packed must be 16-byte aligned");
    return hip_status(mvnerf::launch_pack_net(net_keras, packed, static_cast<hipStream_t>(stream)), "mvnerf_pack_net");
}

int mvnerf_get_rays(const double* m3x3_host, const double* origin_host, const float* u, const float* v, int n_rays,
                    int width, int normalize, float* rays_o, float* rays_d, double* rays_d64,
                    mvnerf_stream_t stream) {
    if (!m3x3_host || !origin_host || !rays_o || !rays_d) return fail(MVNERF_E_ARG, "mvnerf_get_rays: null pointer");
    if ((u == nullptr) != (v == nullptr)) return fail(MVNERF_E_ARG, "mvnerf_get_rays: u and v must both be given or both NULL");
    if (n_rays <= 0 || (!u && width <= 0)) return fail(MVNERF_E_ARG, "mvnerf_get_rays: n_rays=%d width=%d", n_rays, width);
    return hip_status(mvnerf::launch_get_rays(m3x3_host, origin_host, u, v, n_rays, width, normalize, rays_o, rays_d,
                                              rays_d64, static_cast<hipStream_t>(stream)),
                      "mvnerf_get_rays");
}

int mvnerf_stratified_depths(const float* u, int n_rays, int n_samples, double near_, double far_, float* z,
                             mvnerf_stream_t stream) {
    if (!u || !z) return fail(MVNERF_E_ARG, "mvnerf_stratified_depths: null pointer");
    if (n_rays <= 0 || n_samples <= 0) return fail(MVNERF_E_ARG, "mvnerf_stratified_depths: n_rays=%d n_samples=%d", n_rays, n_samples);
    return hip_status(mvnerf::launch_stratified(u, (long)n_rays * n_samples, n_samples, near_, far_, z,
                                                static_cast<hipStream_t>(stream)),
                      "mvnerf_stratified_depths");
}

int mvnerf_field_eval(const float* rays_o, const float* rays_d, const float* z, const float* images,
                      const float* features, const float* intrinsics, const float* extrinsics_inv,
                      const float* packed_net, int B, int V, int R, int S, int H, int W, float* rgbs,
                      int32_t* tap_idx, float* pix, float* embedding, float* acts_per_view, float* acts_fused,
                      void* workspace, mvnerf_stream_t stream) {
    const FieldArgs a = {rays_o, rays_d, z, images, features, nullptr, intrinsics, extrinsics_inv, packed_net, nullptr, B, V, R, S, H, W,
                         rgbs, tap_idx, pix, embedding, acts_per_view, acts_fused, nullptr, workspace};
    return field_pass("mvnerf_field_eval", a, {kFieldFp32, false, MVNERF_E_SHAPE}, stream);
}

size_t mvnerf_texel_table_bytes(int B, int V, int H, int W) {
    if (B <= 0 || V <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * V * H * W * 128 * sizeof(float);
}

int mvnerf_project_texels2(const float* features, const float* packed_net, const float* packed_net_b, int B, int V, int H, int W,
                           float* texel_table, float* texel_table_b, mvnerf_stream_t stream) {
    if (const int rc = texels_check("mvnerf_project_texels", features, packed_net, packed_net_b, B, V, H, W, texel_table, texel_table_b)) return rc;
    return hip_status(mvnerf::launch_project_texels(features, packed_net, packed_net_b, (long)B * V * H * W, texel_table,
                                                    texel_table_b, static_cast<hipStream_t>(stream)),
                      "mvnerf_project_texels");
}

int mvnerf_project_texels(const float* features, const float* packed_net, int B, int V, int H, int W, float* texel_table,
                          mvnerf_stream_t stream) {
    return mvnerf_project_texels2(features, packed_net, nullptr, B, V, H, W, texel_table, nullptr, stream);
}

int mvnerf_field_eval_table(const float* rays_o, const float* rays_d, const float* z, const float* images,
                            const float* features, const float* texel_table, const float* intrinsics,
                            const float* extrinsics_inv, const float* packed_net, int B, int V, int R, int S, int H, int W,
                            float* rgbs, int32_t* tap_idx, float* pix, float* embedding, float* acts_per_view,
                            float* acts_fused, void* workspace, mvnerf_stream_t stream) {
    if (!texel_table) return fail(MVNERF_E_ARG, "mvnerf_field_eval_table: null texel_table");
    const FieldArgs a = {rays_o, rays_d, z, images, features, texel_table, intrinsics, extrinsics_inv, packed_net, nullptr, B, V, R, S, H, W,
                         rgbs, tap_idx, pix, embedding, acts_per_view, acts_fused, nullptr, workspace};
    return field_pass("mvnerf_field_eval", a, {kFieldFp32, false, MVNERF_E_SHAPE}, stream);
}

size_t mvnerf_packed_net_bf16_bytes(void) { return mvnerf::packed_net_bf16_bytes(); }

int mvnerf_pack_net_bf16(const float* net_keras, void* packed16, mvnerf_stream_t stream) {
    if (!net_keras || !packed16) return fail(MVNERF_E_ARG, "mvnerf_pack_net_bf16: null pointer");
    if (!aligned16(packed16)) return fail(MVNERF_E_ALIGN, "mvnerf_pack_net_bf16: packed16 must be 16-byte aligned");
    return hip_status(mvnerf::launch_pack_net_bf16(net_keras, packed16, static_cast<hipStream_t>(stream)), "mvnerf_pack_net_bf16");
}

int mvnerf_project_texels_bf16(const float* features, const void* packed16, const void* packed16_b, int B, int V, int H, int W,
                               float* texel_table, float* texel_table_b, mvnerf_stream_t stream) {
    if (const int rc = texels_check("mvnerf_project_texels_bf16", features, packed16, packed16_b, B, V, H, W, texel_table, texel_table_b)) return rc;
    return hip_status(mvnerf::launch_project_texels_bf16(features, packed16, packed16_b, (long)B * V * H * W, texel_table, texel_table_b,
                                                         static_cast<hipStream_t>(stream)),
                      "mvnerf_project_texels_bf16");
}

int mvnerf_project_texels_bf16maps(const void* features_bf16, const void* packed16, const void* packed16_b, int B, int V, int H, int W,
                                   float* texel_table, float* texel_table_b, mvnerf_stream_t stream) {
    if (const int rc = texels_check("mvnerf_project_texels_bf16maps", features_bf16, packed16, packed16_b, B, V, H, W, texel_table, texel_table_b))
        return rc;
    return hip_status(mvnerf::launch_project_texels_bf16maps(features_bf16, packed16, packed16_b, (long)B * V * H * W, texel_table, texel_table_b,
                                                             static_cast<hipStream_t>(stream)),
                      "mvnerf_project_texels_bf16maps");
}

int mvnerf_field_eval_bf16(const float* rays_o, const float* rays_d, const float* z, const float* images,
                           const float* features, const float* texel_table, const float* intrinsics, const float* extrinsics_inv,
                           const float* packed_net, const void* packed16, int B, int V, int R, int S, int H, int W,
                           float* rgbs, int32_t* tap_idx, float* embedding, float* acts_fused, void* workspace,
                           mvnerf_stream_t stream) {
    const FieldArgs a = {rays_o, rays_d, z, images, features, texel_table, intrinsics, extrinsics_inv, packed_net, packed16, B, V, R, S, H, W,
                         rgbs, tap_idx, nullptr, embedding, nullptr, acts_fused, nullptr, workspace};
    return field_pass("mvnerf_field_eval_bf16", a, {kFieldBf16, false, MVNERF_E_SHAPE}, stream);
}

int mvnerf_field_eval_bf16maps(const float* rays_o, const float* rays_d, const float* z, const float* images,
                               const void* features_bf16, const float* texel_table, const float* intrinsics, const float* extrinsics_inv,
                               const float* packed_net, const void* packed16, int B, int V, int R, int S, int H, int W,
                               float* rgbs, int32_t* tap_idx, float* embedding, float* acts_fused, void* workspace,
                               mvnerf_stream_t stream) {
    const FieldArgs a = {rays_o, rays_d, z, images, static_cast<const float*>(features_bf16), texel_table, intrinsics, extrinsics_inv, packed_net,
                         packed16, B, V, R, S, H, W, rgbs, tap_idx, nullptr, embedding, nullptr, acts_fused, nullptr, workspace};
    return field_pass("mvnerf_field_eval_bf16maps", a, {kFieldBf16Maps, false, MVNERF_E_SHAPE}, stream);
}

size_t mvnerf_packed_net_split_bytes(void) { return mvnerf::packed_net_split_bytes(); }

int mvnerf_pack_net_split(const float* net_keras, void* packed_split, mvnerf_stream_t stream) {
    if (!net_keras || !packed_split) return fail(MVNERF_E_ARG, "mvnerf_pack_net_split: null pointer");
    if (!aligned16(packed_split)) return fail(MVNERF_E_ALIGN, "mvnerf_pack_net_split: packed_split must be 16-byte aligned");
    return hip_status(mvnerf::launch_pack_net_split(net_keras, packed_split, static_cast<hipStream_t>(stream)), "mvnerf_pack_net_split");
}

int mvnerf_field_eval_split(const float* rays_o, const float* rays_d, const float* z, const float* images,
                            const float* features, const float* texel_table, const float* intrinsics, const float* extrinsics_inv,
                            const float* packed_net, const void* packed_split, int B, int V, int R, int S, int H, int W,
                            float* rgbs, int32_t* tap_idx, float* pix, float* embedding, float* acts_per_view, float* acts_fused,
                            void* workspace, mvnerf_stream_t stream) {
    const FieldArgs a = {rays_o, rays_d, z, images, features, texel_table, intrinsics, extrinsics_inv, packed_net, packed_split, B, V, R, S, H, W,
                         rgbs, tap_idx, pix, embedding, acts_per_view, acts_fused, nullptr, workspace};
    return field_pass("mvnerf_field_eval_split", a, {kFieldSplit, false, MVNERF_E_SHAPE}, stream);
}

int mvnerf_field_eval_split_ex(const float* rays_o, const float* rays_d, const float* z, const float* images,
                               const float* features, const float* texel_table, const float* intrinsics, const float* extrinsics_inv,
                               const float* packed_net, const void* packed_split, int B, int V, int R, int S, int H, int W,
                               float* rgbs, int32_t* tap_idx, float* pix, float* embedding, float* acts_per_view, float* acts_fused,
                               void* workspace, int which, float* range_status, mvnerf_stream_t stream) {
    const FieldArgs a = {rays_o, rays_d, z, images, features, texel_table, intrinsics, extrinsics_inv, packed_net, packed_split, B, V, R, S, H, W,
                         rgbs, tap_idx, pix, embedding, acts_per_view, acts_fused, nullptr, workspace};
    return field_pass("mvnerf_field_eval_split_ex", a, {kFieldSplit, false, MVNERF_E_SHAPE}, stream, which, range_status);
}

int mvnerf_net_range(const float* net_keras, float* out2, mvnerf_stream_t stream) {
    if (!net_keras || !out2) return fail(MVNERF_E_ARG, "mvnerf_net_range: null pointer");
    if (!aligned4(out2)) return fail(MVNERF_E_ALIGN, "mvnerf_net_range: out2 must be 4-byte aligned");
    return hip_status(mvnerf::launch_net_range(net_keras, out2, static_cast<hipStream_t>(stream)), "mvnerf_net_range");
}

int mvnerf_composite(const float* z, const float* rgbs, int n_rays, int S, float* rgb, float* depth, float* weights,
                     mvnerf_stream_t stream) {
    if (!z || !rgbs || !rgb || !depth) return fail(MVNERF_E_ARG, "mvnerf_composite: null pointer");
    if (n_rays <= 0) return fail(MVNERF_E_ARG, "mvnerf_composite: n_rays=%d", n_rays);
    if (S % 64 != 0 || S < 64 || S > 256) return fail(MVNERF_E_SHAPE, "mvnerf_composite: S=%d, supported: 64,128,192,256", S);
    if (!aligned16(rgbs)) return fail(MVNERF_E_ALIGN, "mvnerf_composite: rgbs must be 16-byte aligned");
    return hip_status(mvnerf::launch_composite(z, rgbs, n_rays, S, rgb, depth, weights, static_cast<hipStream_t>(stream)),
                      "mvnerf_composite");
}

int mvnerf_resample(const float* z, const float* weights, const float* u_fine, int n_rays, int S, int q7_mode,
                    float* z_all, float* z_fine, int32_t* above, int32_t* below, int32_t* fine_rank,
                    mvnerf_stream_t stream) {
    if (!z || !weights || !u_fine || !z_all) return fail(MVNERF_E_ARG, "mvnerf_resample: null pointer");
    if (n_rays <= 0) return fail(MVNERF_E_ARG, "mvnerf_resample: n_rays=%d", n_rays);
    if (S != 64) return fail(MVNERF_E_SHAPE, "mvnerf_resample: S=%d, only the reference's n_samples=64 is built", S);
    if (q7_mode != MVNERF_Q7_ZERO && q7_mode != MVNERF_Q7_CLAMP) return fail(MVNERF_E_ARG, "mvnerf_resample: q7_mode=%d", q7_mode);
    return hip_status(mvnerf::launch_resample(z, weights, u_fine, n_rays, q7_mode, z_all, z_fine, above, below, fine_rank,
                                              static_cast<hipStream_t>(stream)),
                      "mvnerf_resample");
}

int mvnerf_points_on_rays(const float* rays_o, const float* rays_d, const float* z, int n_rays, int S, float* world,
                          mvnerf_stream_t stream) {
    if (!rays_o || !rays_d || !z || !world) return fail(MVNERF_E_ARG, "mvnerf_points_on_rays: null pointer");
    if (n_rays <= 0 || S <= 0) return fail(MVNERF_E_ARG, "mvnerf_points_on_rays: n_rays=%d S=%d", n_rays, S);
    return hip_status(mvnerf::launch_points_on_rays(rays_o, rays_d, z, (long)n_rays * S, S, world, static_cast<hipStream_t>(stream)),
                      "mvnerf_points_on_rays");
}

int mvnerf_project_points(const float* world, const float* intrinsics, const float* extrinsics_inv, int B, int V, int N,
                          float* pixel_locations, float* camera_points, mvnerf_stream_t stream) {
    if (!world || !intrinsics || !extrinsics_inv || !pixel_locations || !camera_points)
        return fail(MVNERF_E_ARG, "mvnerf_project_points: null pointer");
    if (B <= 0 || V <= 0 || N <= 0) return fail(MVNERF_E_ARG, "mvnerf_project_points: B=%d V=%d N=%d", B, V, N);
    return hip_status(mvnerf::launch_project_points(world, intrinsics, extrinsics_inv, B, V, N, pixel_locations, camera_points,
                                                    static_cast<hipStream_t>(stream)),
                      "mvnerf_project_points");
}

int mvnerf_camera_directions(const float* dirs, const float* extrinsics_inv, int B, int V, int R, float* out,
                             mvnerf_stream_t stream) {
    if (!dirs || !extrinsics_inv || !out) return fail(MVNERF_E_ARG, "mvnerf_camera_directions: null pointer");
    if (B <= 0 || V <= 0 || R <= 0) return fail(MVNERF_E_ARG, "mvnerf_camera_directions: B=%d V=%d R=%d", B, V, R);
    return hip_status(mvnerf::launch_camera_directions(dirs, extrinsics_inv, B, V, R, out, static_cast<hipStream_t>(stream)),
                      "mvnerf_camera_directions");
}

int mvnerf_position_encoding(const float* x, long n_elems, int n_freq, float pos_encoding_freq, float* out,
                             mvnerf_stream_t stream) {
    if (!x || !out) return fail(MVNERF_E_ARG, "mvnerf_position_encoding: null pointer");
    if (n_elems <= 0 || n_freq <= 0 || n_freq > 32) return fail(MVNERF_E_ARG, "mvnerf_position_encoding: n_elems=%ld n_freq=%d", n_elems, n_freq);
    return hip_status(mvnerf::launch_position_encoding(x, n_elems, n_freq, pos_encoding_freq, out, static_cast<hipStream_t>(stream)),
                      "mvnerf_position_encoding");
}

int mvnerf_bilinear_gather(const float* images, const float* features, const float* pixel_locations, int BV, int Q, int H,
                           int W, float* out, int32_t* tap_idx, mvnerf_stream_t stream) {
    if (!images || !features || !pixel_locations || !out) return fail(MVNERF_E_ARG, "mvnerf_bilinear_gather: null pointer");
    if (BV <= 0 || Q <= 0) return fail(MVNERF_E_ARG, "mvnerf_bilinear_gather: BV=%d Q=%d", BV, Q);
    if (H < 2 || W < 2) return fail(MVNERF_E_SHAPE, "mvnerf_bilinear_gather: grid %dx%d, need H,W >= 2", H, W);
    if ((long)BV * H * W >= (1L << 31)) return fail(MVNERF_E_SHAPE, "mvnerf_bilinear_gather: BV*H*W too large for int32 indices");
    return hip_status(mvnerf::launch_bilinear_gather(images, features, pixel_locations, BV, Q, H, W, out, tap_idx,
                                                     static_cast<hipStream_t>(stream)),
                      "mvnerf_bilinear_gather");
}

int mvnerf_sigma_to_alpha(const float* sigma, const float* dists, long n, float* alpha, mvnerf_stream_t stream) {
    if (!sigma || !dists || !alpha) return fail(MVNERF_E_ARG, "mvnerf_sigma_to_alpha: null pointer");
    if (n <= 0) return fail(MVNERF_E_ARG, "mvnerf_sigma_to_alpha: n=%ld", n);
    return hip_status(mvnerf::launch_sigma_to_alpha(sigma, dists, n, alpha, static_cast<hipStream_t>(stream)), "mvnerf_sigma_to_alpha");
}

int mvnerf_sample_pdf(const float* bins, const float* weights, const float* u, int n_rays, int n_bins, int n_samples,
                      int q7_mode, float* samples, int32_t* above, int32_t* below, mvnerf_stream_t stream) {
    if (!bins || !weights || !u || !samples) return fail(MVNERF_E_ARG, "mvnerf_sample_pdf: null pointer");
    if (n_rays <= 0) return fail(MVNERF_E_ARG, "mvnerf_sample_pdf: n_rays=%d", n_rays);
    if (n_bins != 63 || n_samples != 64)
        return fail(MVNERF_E_SHAPE, "mvnerf_sample_pdf: n_bins=%d n_samples=%d, only the reference's 63 bins / 64 samples is built", n_bins, n_samples);
    if (q7_mode != MVNERF_Q7_ZERO && q7_mode != MVNERF_Q7_CLAMP) return fail(MVNERF_E_ARG, "mvnerf_sample_pdf: q7_mode=%d", q7_mode);
    return hip_status(mvnerf::launch_sample_pdf(bins, weights, u, n_rays, q7_mode, samples, above, below, static_cast<hipStream_t>(stream)),
                      "mvnerf_sample_pdf");
}

int mvnerf_readout(const float* embedding, const float* wr, const float* br, long n, float* rgbs, mvnerf_stream_t stream) {
    if (!embedding || !wr || !br || !rgbs) return fail(MVNERF_E_ARG, "mvnerf_readout: null pointer");
    if (n <= 0) return fail(MVNERF_E_ARG, "mvnerf_readout: n=%ld", n);
    return hip_status(mvnerf::launch_readout(embedding, wr, br, n, rgbs, static_cast<hipStream_t>(stream)), "mvnerf_readout");
}

int mvnerf_finish_view(const float* rgb, const float* depth, long n, float* minmax_scratch, uint8_t* rgb8, uint8_t* depth8,
                       mvnerf_stream_t stream) {
    if (!rgb || !depth || !minmax_scratch || !rgb8 || !depth8) return fail(MVNERF_E_ARG, "mvnerf_finish_view: null pointer");
    if (n <= 0) return fail(MVNERF_E_ARG, "mvnerf_finish_view: n=%ld", n);
    return hip_status(mvnerf::launch_finish_view(rgb, depth, n, minmax_scratch, rgb8, depth8, static_cast<hipStream_t>(stream)),
                      "mvnerf_finish_view");
}

// ---- training --------------------------------------------------------------------------------------------
namespace {
constexpr int kBwdMaxWGs = 512;      // resident workgroups of the dW kernels (2 per CU)
constexpr int kFusedBwdWGs = 512;    // fused dX+dW kernel: 2 waves/SIMD by registers -> 2 resident workgroups per CU
static_assert(kBwdMaxWGs == kFusedBwdWGs, "partial_floats() assumes one workgroup budget for every weight-gradient kernel");

// The backward walk through the trunk's residual blocks, 5..0, of mvnerf_field_backward_table and mvnerf_query_vjp: three tile buffers of
// one per-view slot each at the front of `scratch` rotate through the roles g / dh / gn.  grad() is dL/d(output of the next block): the
// caller puts its cotangent there first and finds dL/d(layer-0 output) there after block 0.  block(bi) hands out what the block's two
// Dense launches read and write; what else they are given (weight gradients, partials, amax) and what enters between blocks is the caller's.
struct TrunkBwd {
    struct Block {
        bool fused; long nt;             // blocks 3..5 work on the view mean: n_tiles tiles, the others on view_tiles
        const float *pre_in, *pre_hid;   // stashed pre-activations: the block's input and its hidden layer
        const float *w1, *w2;            // backward weight streams of the first and the second Dense
        float *g, *dh, *gn;              // dL/d(block output), dL/d(hidden), dL/d(block input)
    };
    StashLayout L;
    int B, V;
    const float *stash, *bwd_streams;
    float* scratch;
    int g = 0;
    float* buf(int i) const { return scratch + (size_t)(i % 3) * L.view_stride(); }
    float* grad() const { return buf(g); }
    // In front of block 2 the gradient of the view mean goes back to the views (reduce_mean, layers.py:368-370): the one launch in here.
    hipError_t block(int bi, Block* b, hipStream_t st) {
        if (bi == 2 && V > 1) {
            const hipError_t e = mvnerf::launch_view_broadcast(buf(g), V, L.n_tiles / B, L.n_tiles, buf(g + 1), st);
            if (e != hipSuccess) return e;
            g = (g + 1) % 3;
        }
        b->fused = bi >= 3;
        b->nt = b->fused ? L.n_tiles : L.view_tiles;
        b->pre_in = stash + (b->fused ? L.fused_slot(2 * (bi - 3)) : L.view_slot(2 * bi));
        b->pre_hid = stash + (b->fused ? L.fused_slot(2 * (bi - 3) + 1) : L.view_slot(2 * bi + 1));
        b->w1 = bwd_streams + (size_t)(2 * bi) * mvnerf::kHiddenWFloats; b->w2 = b->w1 + mvnerf::kHiddenWFloats;
        b->g = buf(g); b->dh = buf(g + 1); b->gn = buf(g + 2);
        g = (g + 2) % 3;
        return hipSuccess;
    }
};
}  // namespace

size_t mvnerf_stash_bytes(int B, int V, int R, int S) {
    if (B <= 0 || V <= 0 || R <= 0 || S <= 0) return 0;
    return StashLayout(B, V, (long)R * S).bytes();
}

// Per-workgroup partials of a weight-gradient span, summed in workgroup order by reduce_partials_kernel.  The three users:
// dw0_split8_kernel (layer 0: 379 x 128 + 128 floats per workgroup, kBwdMaxWGs / 2 = 256 workgroups at most, never more than there are
// view tiles), dense_bwd_split8_kernel (128 x 128 + 128, kFusedBwdWGs / 2) and the read-out's dw_tile_kernel (516 floats, kBwdMaxWGs).
// Behind them: 14 x 64 floats, max |g| of the gradient tensor each layer launch of the training backward reads (the power-of-two scale
// of its fp16 cut; train_ops.hip, MVT_BWD_F16).
constexpr int kAmaxTensors = 14;
static size_t partial_only_floats(long n_tiles, int V) {
    const long wg0 = n_tiles * V < kBwdMaxWGs / 2 ? n_tiles * V : kBwdMaxWGs / 2;
    const long wgr = n_tiles < kBwdMaxWGs ? n_tiles : kBwdMaxWGs;
    const size_t a = (size_t)wg0 * (mvnerf::kIn * mvnerf::kHidden + mvnerf::kHidden), b = (size_t)wgr * 516;
    return ((a > b ? a : b) + 3) & ~(size_t)3;
}
static size_t partial_floats(long n_tiles, int V) { return partial_only_floats(n_tiles, V) + (size_t)kAmaxTensors * mvnerf::kBwdAmaxSlots; }
std::atomic<int> g_deterministic{0};

size_t mvnerf_field_backward_scratch_bytes(int B, int V, int R, int S) {
    if (B <= 0 || V <= 0 || R <= 0 || S <= 0) return 0;
    const long n_tiles = StashLayout(B, V, (long)R * S).n_tiles;          // three tile buffers, the read-out's cotangent tile, the partials
    return ((size_t)n_tiles * ((size_t)3 * V * 128 + 32) * 32 + partial_floats(n_tiles, V)) * sizeof(float);
}

int mvnerf_set_deterministic(int on) { return g_deterministic.exchange(on ? 1 : 0); }

int mvnerf_set_split_kernel(int which) {
    const int prev = mvnerf::set_split_kernel(which);
    if (prev < 0) return fail(MVNERF_E_ARG, "mvnerf_set_split_kernel: which=%d (0 f16x3, 1 bf16x6, 2 bf16x6 as 32x32x16)", which);
    return prev;
}

int mvnerf_field_eval_stash(const float* rays_o, const float* rays_d, const float* z, const float* images,
                            const float* features, const float* texel_table, const float* intrinsics,
                            const float* extrinsics_inv, const float* packed_net, int B, int V, int R, int S, int H, int W,
                            float* rgbs, float* stash, void* workspace, mvnerf_stream_t stream) {
    const FieldArgs a = {rays_o, rays_d, z, images, features, texel_table, intrinsics, extrinsics_inv, packed_net, nullptr, B, V, R, S, H, W,
                         rgbs, nullptr, nullptr, nullptr, nullptr, nullptr, stash, workspace};
    return field_pass("mvnerf_field_eval_stash", a, {kFieldFp32, true, MVNERF_E_ARG}, stream);
}

int mvnerf_field_eval_stash_split(const float* rays_o, const float* rays_d, const float* z, const float* images,
                                  const float* features, const float* texel_table, const float* intrinsics,
                                  const float* extrinsics_inv, const float* packed_net, const void* packed_split, int B, int V, int R,
                                  int S, int H, int W, float* rgbs, float* stash, void* workspace, mvnerf_stream_t stream) {
    const FieldArgs a = {rays_o, rays_d, z, images, features, texel_table, intrinsics, extrinsics_inv, packed_net, packed_split, B, V, R, S, H, W,
                         rgbs, nullptr, nullptr, nullptr, nullptr, nullptr, stash, workspace};
    return field_pass("mvnerf_field_eval_stash_split", a, {kFieldSplit, true, MVNERF_E_ARG}, stream);
}

int mvnerf_field_eval_stash_split_ex(const float* rays_o, const float* rays_d, const float* z, const float* images,
                                     const float* features, const float* texel_table, const float* intrinsics,
                                     const float* extrinsics_inv, const float* packed_net, const void* packed_split, int B, int V, int R,
                                     int S, int H, int W, float* rgbs, float* stash, void* workspace, int which, float* range_status,
                                     mvnerf_stream_t stream) {
    const FieldArgs a = {rays_o, rays_d, z, images, features, texel_table, intrinsics, extrinsics_inv, packed_net, packed_split, B, V, R, S, H, W,
                         rgbs, nullptr, nullptr, nullptr, nullptr, nullptr, stash, workspace};
    return field_pass("mvnerf_field_eval_stash_split_ex", a, {kFieldSplit, true, MVNERF_E_ARG}, stream, which, range_status);
}

int mvnerf_pack_bwd_streams(const float* net_keras, float* bwd_streams, mvnerf_stream_t stream) {
    if (!net_keras || !bwd_streams) return fail(MVNERF_E_ARG, "mvnerf_pack_bwd_streams: null pointer");
    if (!aligned16(bwd_streams)) return fail(MVNERF_E_ALIGN, "mvnerf_pack_bwd_streams: bwd_streams must be 16-byte aligned");
    return hip_status(mvnerf::launch_pack_bwd_streams(net_keras, bwd_streams, static_cast<hipStream_t>(stream)), "mvnerf_pack_bwd_streams");
}

int mvnerf_mse_grad(const float* pred, const float* label, long n, float* d_pred, float* loss, mvnerf_stream_t stream) {
    if (!pred || !label || !d_pred || !loss) return fail(MVNERF_E_ARG, "mvnerf_mse_grad: null pointer");
    if (n <= 0) return fail(MVNERF_E_ARG, "mvnerf_mse_grad: n=%ld", n);
    return hip_status(mvnerf::launch_mse_grad(pred, label, n, d_pred, loss, static_cast<hipStream_t>(stream)), "mvnerf_mse_grad");
}

int mvnerf_composite_bwd(const float* z, const float* rgbs, const float* d_rgb, const float* d_depth,
                         const float* d_weights, int n_rays, int S, float* d_rgbs, float* d_z, mvnerf_stream_t stream) {
    if (!z || !rgbs || !d_rgb || !d_rgbs) return fail(MVNERF_E_ARG, "mvnerf_composite_bwd: null pointer");
    if (n_rays <= 0) return fail(MVNERF_E_ARG, "mvnerf_composite_bwd: n_rays=%d", n_rays);
    if (S != 64 && S != 128) return fail(MVNERF_E_SHAPE, "mvnerf_composite_bwd: S=%d, supported: 64, 128", S);
    if (!aligned16(rgbs) || !aligned16(d_rgbs)) return fail(MVNERF_E_ALIGN, "mvnerf_composite_bwd: rgbs, d_rgbs must be 16-byte aligned");
    return hip_status(mvnerf::launch_composite_bwd(z, rgbs, d_rgb, d_depth, d_weights, n_rays, S, d_rgbs, d_z,
                                                   static_cast<hipStream_t>(stream)),
                      "mvnerf_composite_bwd");
}

int mvnerf_resample_bwd(const float* z, const float* weights, const float* u_fine, const int32_t* fine_rank,
                        const float* d_z_all, int n_rays, int S, int q7_mode, float* d_weights, mvnerf_stream_t stream) {
    if (!z || !weights || !u_fine || !fine_rank || !d_z_all || !d_weights) return fail(MVNERF_E_ARG, "mvnerf_resample_bwd: null pointer");
    if (n_rays <= 0) return fail(MVNERF_E_ARG, "mvnerf_resample_bwd: n_rays=%d", n_rays);
    if (S != 64) return fail(MVNERF_E_SHAPE, "mvnerf_resample_bwd: S=%d, only the reference's n_samples=64 is built", S);
    return hip_status(mvnerf::launch_resample_bwd(z, weights, u_fine, fine_rank, d_z_all, n_rays, q7_mode, d_weights,
                                                  static_cast<hipStream_t>(stream)),
                      "mvnerf_resample_bwd");
}

int mvnerf_field_backward(const float* rays_o, const float* rays_d, const float* z, const float* images,
                          const float* features, const float* intrinsics, const float* extrinsics_inv,
                          const float* net_keras, const float* bwd_streams, const float* stash, const float* rgbs,
                          const float* d_rgbs, int B, int V, int R, int S, int H, int W, void* scratch, float* grad,
                          float* d_z, float* d_features, mvnerf_stream_t stream) {
    return mvnerf_field_backward_table(rays_o, rays_d, z, images, features, nullptr, nullptr, intrinsics, extrinsics_inv, net_keras,
                                       bwd_streams, stash, rgbs, d_rgbs, B, V, R, S, H, W, scratch, grad, d_z, d_features, stream);
}

int mvnerf_field_backward_table(const float* rays_o, const float* rays_d, const float* z, const float* images,
                                const float* features, const float* texel_table, float* texel_grad, const float* intrinsics,
                                const float* extrinsics_inv, const float* net_keras, const float* bwd_streams, const float* stash,
                                const float* rgbs, const float* d_rgbs, int B, int V, int R, int S, int H, int W, void* scratch,
                                float* grad, float* d_z, float* d_features, mvnerf_stream_t stream) {
    using namespace mvnerf;
    if ((texel_table && !aligned16(texel_table)) || (texel_grad && !aligned16(texel_grad)))
        return fail(MVNERF_E_ALIGN, "mvnerf_field_backward: texel_table, texel_grad must be 16-byte aligned");
    if (texel_grad && !texel_table) return fail(MVNERF_E_ARG, "mvnerf_field_backward: texel_grad needs texel_table");
    if (!rays_o || !rays_d || !z || !images || !features || !intrinsics || !extrinsics_inv || !net_keras || !bwd_streams ||
        !stash || !rgbs || !d_rgbs || !scratch || !grad)
        return fail(MVNERF_E_ARG, "mvnerf_field_backward: null pointer");
    if (B <= 0 || V <= 0 || R <= 0 || S <= 0 || H < 2 || W < 2) return fail(MVNERF_E_ARG, "mvnerf_field_backward: bad sizes");
    if (V > 1 && ((long)R * S) % 32 != 0) return fail(MVNERF_E_SHAPE, "mvnerf_field_backward: R*S must be a multiple of 32 when V > 1");
    if (!aligned16(net_keras) || !aligned16(bwd_streams) || !aligned16(stash) || !aligned16(rgbs) || !aligned16(d_rgbs) || !aligned16(scratch))
        return fail(MVNERF_E_ALIGN, "mvnerf_field_backward: net_keras, bwd_streams, stash, rgbs, d_rgbs, scratch must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const char* const who = "mvnerf_field_backward";
    const StashLayout L(B, V, (long)R * S);
    const long total = L.total, n_tiles = L.n_tiles;
    TrunkBwd walk = {L, B, V, stash, bwd_streams, static_cast<float*>(scratch)};
    float* do_tl = static_cast<float*>(scratch) + 3 * L.view_stride();
    // per-workgroup partials of every weight-gradient span, added in workgroup order by reduce_partials_kernel: bit-identical from run
    // to run AND faster than fp32 atomics onto the same addresses (7.54 vs 7.60 ms per step at cfg2), so it is the only mode since
    // round 2; mvnerf_set_deterministic is kept for its callers and has no effect on the weight gradients any more
    float* part = do_tl + (size_t)n_tiles * 32 * 32;
    // max |g| slots of the 13 gradient tensors of the chain (zeroed here, filled by each tensor's producer)
    float* amax = part + partial_only_floats(n_tiles, V);
    MV_HIP(mvnerf::launch_zero(amax, (size_t)kAmaxTensors * mvnerf::kBwdAmaxSlots * sizeof(float), st), who);
    int am = 0;                                        // amax + 64 am belongs to the block's g
    auto amax_of = [&](int k) { return amax + (size_t)k * mvnerf::kBwdAmaxSlots; };
    // read-out
    MV_HIP(launch_readout_bwd(stash + L.fused_slot(6), rgbs, d_rgbs, net_keras + kKerasWr, total, n_tiles, do_tl, walk.grad(), st, amax_of(0)), who);
    MV_HIP(launch_dw_tile(stash + L.fused_slot(6), 1, do_tl, 32, n_tiles, grad + kKerasWr, 4, 4, grad + kKerasBr, kBwdMaxWGs, part, st), who);
    for (int bi = 5; bi >= 0; --bi) {
        TrunkBwd::Block b;
        MV_HIP(walk.block(bi, &b, st), who);
        float* gb = grad + kKerasBlocks + bi * kKerasBlockStride;
        // second Dense of the block: out = x_in + W2^T relu(hid) + b2      (dX and dW in one pass over the tiles)
        MV_HIP(launch_dense_bwd_fused(b.g, b.pre_hid, b.w2, nullptr, b.dh, b.nt, gb + kHidden * kHidden + kHidden, gb + 2 * kHidden * kHidden + kHidden,
                                      kFusedBwdWGs, part, st, amax_of(am), amax_of(am + 1)), who);
        // first Dense: hid = W1^T relu(x_in) + b1 ; the identity branch adds dL/d(out) back
        MV_HIP(launch_dense_bwd_fused(b.dh, b.pre_in, b.w1, b.g, b.gn, b.nt, gb, gb + kHidden * kHidden, kFusedBwdWGs, part, st, amax_of(am + 1),
                                      amax_of(am + 2)), who);
        am += 2;                                       // (the view broadcast scales by 1 / V: its output keeps its input's bound)
    }
    // layer 0 (inputs recomputed)
    const float* g0 = walk.grad();                         // dL/d(layer-0 output)
    FieldParams p = {};
    p.rays_o = rays_o; p.rays_d = rays_d; p.z = z; p.images = images; p.features = features;
    p.k4 = intrinsics; p.einv = extrinsics_inv;
    p.B = B; p.V = V; p.R = R; p.S = S; p.H = H; p.W = W; p.total = total; p.n_tiles = n_tiles;
    p.texel_table = texel_table;                           // only the sample-position gradient uses it (launch_field_dz)
    p.net = net_keras;                                     // (Keras layout here: field_dz_table_kernel reads W0's rgb rows from it)
    MV_HIP(launch_dw0(p, g0, grad + kKerasW0, grad + kKerasB0, kBwdMaxWGs, part, st, amax_of(am)), who);
    // d_features through the texel table (texel_grad given): the samples' g0 is scattered onto the 128-channel table gradient and W0 is
    // applied once per texel afterwards; the sample-position gradient then takes the table path as well
    const bool via_table = d_features && texel_table && texel_grad;
    if (via_table) {
        const long n_texels = (long)B * V * H * W;
        MV_HIP(mvnerf::launch_zero(texel_grad, (size_t)n_texels * 128 * sizeof(float), st), who);
        MV_HIP(launch_texel_scatter(p, g0, texel_grad, st), who);
        MV_HIP(launch_texel_grad_to_features(texel_grad, net_keras + kKerasW0 + 123 * kHidden, n_texels, d_features, st), who);
    }
    if (d_z || (d_features && !via_table))
        MV_HIP(launch_field_dz(p, g0, bwd_streams + (size_t)12 * kHiddenWFloats, d_z, nullptr, nullptr, via_table ? nullptr : d_features, st), who);
    return 0;
}

static bool gemm_nt_shape_ok(int M, int N, int K) { return M > 0 && N > 0 && K > 0 && M % 32 == 0 && N % 64 == 0 && K % 8 == 0; }

size_t mvnerf_gemm_nt_scratch_bytes(int M, int N, int K) {
    if (!gemm_nt_shape_ok(M, N, K)) return 0;
    const int splits = mvnerf::gemm_nt_splits(M, N, K);
    return splits > 1 ? (size_t)splits * M * N * sizeof(float) : 0;
}

static int gemm_nt_impl(const char* who, const float* a, const float* bt, const float* bias, float* c, int M, int N, int K, void* scratch,
                        mvnerf_stream_t stream) {
    if (!a || !bt || !c) return fail(MVNERF_E_ARG, "%s: null pointer", who);
    if (!gemm_nt_shape_ok(M, N, K))
        return fail(MVNERF_E_SHAPE, "%s: M=%d N=%d K=%d, needs M %% 32 == 0, N %% 64 == 0, K %% 8 == 0", who, M, N, K);
    if (!aligned16(a) || !aligned16(bt) || !aligned16(c) || (scratch && !aligned16(scratch)) || (bias && !aligned16(bias)))
        return fail(MVNERF_E_ALIGN, "%s: a, bt, bias, c, scratch must be 16-byte aligned", who);
    if (mvnerf_gemm_nt_scratch_bytes(M, N, K) && !scratch) return fail(MVNERF_E_ARG, "%s: this shape needs scratch", who);
    return hip_status(mvnerf::launch_gemm_nt_f32(a, bt, bias, c, M, N, K, static_cast<float*>(scratch), static_cast<hipStream_t>(stream)), who);
}

int mvnerf_gemm_nt(const float* a, const float* bt, float* c, int M, int N, int K, void* scratch, mvnerf_stream_t stream) {
    return gemm_nt_impl("mvnerf_gemm_nt", a, bt, nullptr, c, M, N, K, scratch, stream);
}

int mvnerf_gemm_nt_bias(const float* a, const float* bt, const float* bias, float* c, int M, int N, int K, void* scratch,
                        mvnerf_stream_t stream) {
    if (!bias) return fail(MVNERF_E_ARG, "mvnerf_gemm_nt_bias: null pointer");
    return gemm_nt_impl("mvnerf_gemm_nt_bias", a, bt, bias, c, M, N, K, scratch, stream);
}

static bool gemm_tn_shape_ok(int M, int N, int K) { return M > 0 && N > 0 && K > 0 && M % 8 == 0 && N % 32 == 0 && K % 64 == 0; }

size_t mvnerf_gemm_tn_scratch_bytes(int M, int N, int K) {
    if (!gemm_tn_shape_ok(M, N, K)) return 0;
    const int splits = mvnerf::gemm_tn_splits(M, N, K);
    return splits > 1 ? (size_t)splits * N * K * sizeof(float) : 0;
}

int mvnerf_gemm_tn(const float* g, const float* a, float* c, int M, int N, int K, void* scratch, mvnerf_stream_t stream) {
    if (!g || !a || !c) return fail(MVNERF_E_ARG, "mvnerf_gemm_tn: null pointer");
    if (!gemm_tn_shape_ok(M, N, K))
        return fail(MVNERF_E_SHAPE, "mvnerf_gemm_tn: M=%d N=%d K=%d, needs M %% 8 == 0, N %% 32 == 0, K %% 64 == 0", M, N, K);
    if (!aligned16(g) || !aligned16(a) || !aligned16(c) || (scratch && !aligned16(scratch)))
        return fail(MVNERF_E_ALIGN, "mvnerf_gemm_tn: g, a, c, scratch must be 16-byte aligned");
    if (mvnerf_gemm_tn_scratch_bytes(M, N, K) && !scratch) return fail(MVNERF_E_ARG, "mvnerf_gemm_tn: this shape needs scratch");
    return hip_status(mvnerf::launch_gemm_tn_f32(g, a, c, M, N, K, static_cast<float*>(scratch), static_cast<hipStream_t>(stream)),
                      "mvnerf_gemm_tn");
}

size_t mvnerf_gemm_tn_batched_scratch_bytes(int M, int N, int K, int batch, int with_colsum) {
    if (!gemm_tn_shape_ok(M, N, K) || batch <= 0) return 0;
    return mvnerf::gemm_tn_batched_scratch_floats(M, N, K, batch, with_colsum != 0) * sizeof(float);
}

int mvnerf_gemm_tn_batched(const mvnerf_gemm_tn_batch* q, float* c, float* colsum, int M, int N, int K, int batch, void* scratch,
                           mvnerf_stream_t stream) {
    if (!q || !q->g || !q->a || !c) return fail(MVNERF_E_ARG, "mvnerf_gemm_tn_batched: null pointer");
    if ((q->g2 == nullptr) != (q->a2 == nullptr)) return fail(MVNERF_E_ARG, "mvnerf_gemm_tn_batched: g2 and a2 come together");
    if (!gemm_tn_shape_ok(M, N, K) || batch <= 0)
        return fail(MVNERF_E_SHAPE, "mvnerf_gemm_tn_batched: M=%d N=%d K=%d batch=%d, needs M %% 8 == 0, N %% 32 == 0, K %% 64 == 0", M, N, K, batch);
    if (q->ldg < N || q->lda < K || (q->g2 && (q->ldg2 < N || q->lda2 < K)))
        return fail(MVNERF_E_SHAPE, "mvnerf_gemm_tn_batched: row strides ldg=%d lda=%d ldg2=%d lda2=%d below N=%d / K=%d", q->ldg, q->lda, q->ldg2, q->lda2, N, K);
    if (q->colsum_of < 0 || q->colsum_of > 2 || (q->colsum_of == 2 && !q->g2) || (q->colsum_of != 0 && !colsum))
        return fail(MVNERF_E_ARG, "mvnerf_gemm_tn_batched: colsum_of=%d without its operand or output", q->colsum_of);
    if (!aligned16(c) || (colsum && !aligned16(colsum)) || (scratch && !aligned16(scratch)))
        return fail(MVNERF_E_ALIGN, "mvnerf_gemm_tn_batched: c, colsum, scratch must be 16-byte aligned");
    if (mvnerf_gemm_tn_batched_scratch_bytes(M, N, K, batch, q->colsum_of != 0) && !scratch)
        return fail(MVNERF_E_ARG, "mvnerf_gemm_tn_batched: this shape needs scratch");
    mvnerf::TnBatchArgs a;
    a.G = q->g; a.A = q->a; a.G2 = q->g2; a.A2 = q->a2;
    a.g_bstride = q->g_batch_stride; a.a_bstride = q->a_batch_stride; a.g2_bstride = q->g2_batch_stride; a.a2_bstride = q->a2_batch_stride;
    a.ldg = q->ldg; a.lda = q->lda; a.ldg2 = q->ldg2; a.lda2 = q->lda2;
    a.colsum_of = q->colsum_of;
    return hip_status(mvnerf::launch_gemm_tn_batched(a, c, colsum, M, N, K, batch, static_cast<float*>(scratch), static_cast<hipStream_t>(stream)),
                      "mvnerf_gemm_tn_batched");
}

// ---- the trunk as a differentiable field on query points --------------------------------------
size_t mvnerf_query_workspace_bytes(int B, int V, int N) {
    if (B <= 0 || V <= 0 || N <= 0) return 0;
    return (size_t)2 * B * V * N * 128 * sizeof(float);        // layer-0 seed and its tangent per (view, point)
}

int mvnerf_query_jvp(const float* points, const float* dirs, const float* t_points, const float* t_dirs,
                     const float* images, const float* features, const float* intrinsics, const float* extrinsics_inv,
                     const float* packed_net, int B, int V, int N, int H, int W, float* acts, float* t_acts, void* workspace,
                     mvnerf_stream_t stream) {
    if (!points || !dirs || !t_points || !t_dirs || !images || !features || !intrinsics || !extrinsics_inv || !packed_net ||
        !t_acts || !workspace)
        return fail(MVNERF_E_ARG, "mvnerf_query_jvp: null pointer");
    if (B <= 0 || V <= 0 || N <= 0) return fail(MVNERF_E_ARG, "mvnerf_query_jvp: B=%d V=%d N=%d", B, V, N);
    if (H < 2 || W < 2) return fail(MVNERF_E_SHAPE, "mvnerf_query_jvp: source image %dx%d, need H,W >= 2", H, W);
    if ((long)B * N >= (1L << 31) || (long)B * V * H * W >= (1L << 31)) return fail(MVNERF_E_SHAPE, "mvnerf_query_jvp: sizes too large for int32 indices");
    if (!aligned16(features) || !aligned16(packed_net) || !aligned16(t_acts) || (acts && !aligned16(acts)) || !aligned16(workspace))
        return fail(MVNERF_E_ALIGN, "mvnerf_query_jvp: features, packed_net, acts, t_acts, workspace must be 16-byte aligned");
    mvnerf::FieldParams p = {};
    p.rays_o = points; p.rays_d = dirs; p.z = nullptr; p.t_o = t_points; p.t_d = t_dirs;
    p.images = images; p.features = features; p.k4 = intrinsics; p.einv = extrinsics_inv; p.net = packed_net;
    p.acts_fused = acts; p.t_acts = t_acts;
    p.dir_bias = static_cast<float*>(workspace);
    p.dir_tan = p.dir_bias + (size_t)B * V * N * 128;
    p.B = B; p.V = V; p.R = N; p.S = 1; p.H = H; p.W = W;
    p.total = (long)B * N;
    p.n_tiles = (p.total + 31) / 32;
    return hip_status(mvnerf::launch_field_jvp(p, static_cast<hipStream_t>(stream)), "mvnerf_query_jvp");
}

size_t mvnerf_query_vjp_scratch_bytes(int B, int V, int N) {
    if (B <= 0 || V <= 0 || N <= 0) return 0;
    return (size_t)3 * StashLayout(B, V, N).view_stride() * sizeof(float);        // the three rotating tile buffers
}

int mvnerf_query_vjp(const float* points, const float* dirs, const float* images, const float* features,
                     const float* intrinsics, const float* extrinsics_inv, const float* bwd_streams, const float* stash,
                     const float* g_acts, int B, int V, int N, int H, int W, void* scratch, float* d_points, float* d_dirs,
                     mvnerf_stream_t stream) {
    using namespace mvnerf;
    if (!points || !dirs || !images || !features || !intrinsics || !extrinsics_inv || !bwd_streams || !stash || !g_acts ||
        !scratch || !d_points || !d_dirs)
        return fail(MVNERF_E_ARG, "mvnerf_query_vjp: null pointer");
    if (B <= 0 || V <= 0 || N <= 0 || H < 2 || W < 2) return fail(MVNERF_E_ARG, "mvnerf_query_vjp: bad sizes");
    if (V > 1 && N % 32 != 0) return fail(MVNERF_E_SHAPE, "mvnerf_query_vjp: N=%d must be a multiple of 32 when V > 1", N);
    if (!aligned16(features) || !aligned16(bwd_streams) || !aligned16(stash) || !aligned16(g_acts) || !aligned16(scratch))
        return fail(MVNERF_E_ALIGN, "mvnerf_query_vjp: features, bwd_streams, stash, g_acts, scratch must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const char* const who = "mvnerf_query_vjp";
    const StashLayout L(B, V, N);
    const long total = L.total, n_tiles = L.n_tiles;
    TrunkBwd walk = {L, B, V, stash, bwd_streams, static_cast<float*>(scratch)};
    MV_HIP(launch_zero(d_points, (size_t)total * 3 * sizeof(float), st), who);
    MV_HIP(launch_zero(d_dirs, (size_t)total * 3 * sizeof(float), st), who);
    // the cotangents of u3, u2, u1 and the view mean enter where those tensors are produced
    MV_HIP(launch_rows_to_tl(g_acts + (size_t)3 * total * 128, total, n_tiles, 0, walk.grad(), st), who);
    for (int bi = 5; bi >= 0; --bi) {
        TrunkBwd::Block b;
        MV_HIP(walk.block(bi, &b, st), who);
        MV_HIP(launch_dense_bwd_fused(b.g, b.pre_hid, b.w2, nullptr, b.dh, b.nt, nullptr, nullptr, kFusedBwdWGs, nullptr, st), who);
        MV_HIP(launch_dense_bwd_fused(b.dh, b.pre_in, b.w1, b.g, b.gn, b.nt, nullptr, nullptr, kFusedBwdWGs, nullptr, st), who);
        if (b.fused) MV_HIP(launch_rows_to_tl(g_acts + (size_t)(bi - 3) * total * 128, total, n_tiles, 1, b.gn, st), who);
    }
    FieldParams p = {};
    p.rays_o = points; p.rays_d = dirs; p.z = nullptr; p.images = images; p.features = features;
    p.k4 = intrinsics; p.einv = extrinsics_inv;
    p.B = B; p.V = V; p.R = N; p.S = 1; p.H = H; p.W = W; p.total = total; p.n_tiles = n_tiles;
    MV_HIP(launch_field_dz(p, walk.grad(), bwd_streams + (size_t)12 * kHiddenWFloats, nullptr, d_points, d_dirs, nullptr, st), who);
    return 0;
}

// ---- the same field on the bf16 matrix pipe: relu bits instead of a stash, one launch for the twelve hidden layers (query_bf16.hip) ----
size_t mvnerf_relu_bits_bytes(int B, int V, int N) {
    if (B <= 0 || V <= 0 || N <= 0) return 0;
    const StashLayout L(B, V, N);
    return (size_t)(L.view_tiles + L.n_tiles) * 6 * 512;                  // 6 slots per view tile and per tile, 1 bit x 128 x 32 each
}

size_t mvnerf_bwd_streams_bf16_bytes(void) { return mvnerf::bwd_streams_bf16_bytes(); }

int mvnerf_pack_bwd_streams_bf16(const float* net_keras, void* bwd16, mvnerf_stream_t stream) {
    if (!net_keras || !bwd16) return fail(MVNERF_E_ARG, "mvnerf_pack_bwd_streams_bf16: null pointer");
    if (!aligned16(bwd16)) return fail(MVNERF_E_ALIGN, "mvnerf_pack_bwd_streams_bf16: bwd16 must be 16-byte aligned");
    return hip_status(mvnerf::launch_pack_bwd_streams_bf16(net_keras, bwd16, static_cast<hipStream_t>(stream)), "mvnerf_pack_bwd_streams_bf16");
}

namespace {
// sizes of the three bf16 query entry points: 0 or the error code
int query_bf16_sizes(const char* who, int B, int V, int N) {
    if (B <= 0 || V <= 0 || N <= 0) return fail(MVNERF_E_ARG, "%s: bad sizes", who);
    if (V > 1 && N % 32 != 0) return fail(MVNERF_E_SHAPE, "%s: N=%d must be a multiple of 32 when V > 1", who, N);
    const StashLayout L(B, V, N);
    if (L.total >= (1L << 31) || L.view_tiles >= (1L << 18))              // g0 tiles are addressed with 32-bit byte offsets (16 KiB per tile)
        return fail(MVNERF_E_SHAPE, "%s: V*B*N/32 = %ld tiles, at most 262143", who, L.view_tiles);
    return 0;
}
}  // namespace

int mvnerf_query_stash_bf16(const float* points, const float* dirs, const float* images, const float* features, const float* intrinsics,
                            const float* extrinsics_inv, const float* packed_net, const void* packed16, int B, int V, int N, int H, int W,
                            float* acts, void* relu_bits, void* workspace, mvnerf_stream_t stream) {
    const char* const who = "mvnerf_query_stash_bf16";
    if (!points || !dirs || !images || !features || !intrinsics || !extrinsics_inv || !packed_net || !packed16 || !acts || !relu_bits ||
        !workspace)
        return fail(MVNERF_E_ARG, "%s: null pointer", who);
    if (H < 2 || W < 2) return fail(MVNERF_E_ARG, "%s: bad sizes", who);
    if (const int rc = query_bf16_sizes(who, B, V, N)) return rc;
    if ((long)B * V * H * W >= (1L << 31)) return fail(MVNERF_E_SHAPE, "%s: B*V*H*W too large for int32 indices", who);
    if (!aligned16(features) || !aligned16(packed_net) || !aligned16(packed16) || !aligned16(acts) || !aligned16(relu_bits) ||
        !aligned16(workspace))
        return fail(MVNERF_E_ALIGN, "%s: features, packed nets, acts, relu_bits, workspace must be 16-byte aligned", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const StashLayout L(B, V, N);
    // workspace (mvnerf_query_workspace_bytes): the layer-0 seeds, then the field pass's z = 0 and its read-out nobody asked for
    float* const ws = static_cast<float*>(workspace);
    float* const z = ws + (size_t)B * V * N * 128;
    float* const rgbs = z + ((L.total + 3) & ~3L);
    MV_HIP(mvnerf::launch_zero(z, (size_t)L.total * sizeof(float), st), who);
    mvnerf::FieldParams p = {};
    p.rays_o = points; p.rays_d = dirs; p.z = z; p.images = images; p.features = features;
    p.k4 = intrinsics; p.einv = extrinsics_inv; p.net = packed_net; p.rgbs = rgbs; p.acts_fused = acts; p.dir_bias = ws;
    p.B = B; p.V = V; p.R = N; p.S = 1; p.H = H; p.W = W; p.total = L.total; p.n_tiles = L.n_tiles;
    return hip_status(mvnerf::launch_field_eval_bf16_bits(p, packed16, relu_bits, st), who);
}

int mvnerf_trunk_vjp_bf16(const void* bwd16, const void* relu_bits, const float* g_acts, int B, int V, int N, float* g0_tl,
                          mvnerf_stream_t stream) {
    const char* const who = "mvnerf_trunk_vjp_bf16";
    if (!bwd16 || !relu_bits || !g_acts || !g0_tl) return fail(MVNERF_E_ARG, "%s: null pointer", who);
    if (const int rc = query_bf16_sizes(who, B, V, N)) return rc;
    if (!aligned16(bwd16) || !aligned16(relu_bits) || !aligned16(g_acts) || !aligned16(g0_tl))
        return fail(MVNERF_E_ALIGN, "%s: bwd16, relu_bits, g_acts, g0_tl must be 16-byte aligned", who);
    const StashLayout L(B, V, N);
    return hip_status(mvnerf::launch_trunk_vjp_bf16(bwd16, relu_bits, g_acts, B, V, L.total, L.n_tiles, g0_tl, static_cast<hipStream_t>(stream)), who);
}

size_t mvnerf_query_vjp_bf16_scratch_bytes(int B, int V, int N) {
    if (B <= 0 || V <= 0 || N <= 0) return 0;
    return (size_t)StashLayout(B, V, N).view_stride() * sizeof(float);            // g0, one tile buffer
}

int mvnerf_query_vjp_bf16(const float* points, const float* dirs, const float* images, const float* features, const float* intrinsics,
                          const float* extrinsics_inv, const float* bwd_streams, const void* bwd16, const void* relu_bits,
                          const float* g_acts, int B, int V, int N, int H, int W, void* scratch, float* d_points, float* d_dirs,
                          mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* const who = "mvnerf_query_vjp_bf16";
    if (!points || !dirs || !images || !features || !intrinsics || !extrinsics_inv || !bwd_streams || !bwd16 || !relu_bits || !g_acts ||
        !scratch || !d_points || !d_dirs)
        return fail(MVNERF_E_ARG, "%s: null pointer", who);
    if (H < 2 || W < 2) return fail(MVNERF_E_ARG, "%s: bad sizes", who);
    if (const int rc = query_bf16_sizes(who, B, V, N)) return rc;
    if (!aligned16(features) || !aligned16(bwd_streams) || !aligned16(bwd16) || !aligned16(relu_bits) || !aligned16(g_acts) ||
        !aligned16(scratch))
        return fail(MVNERF_E_ALIGN, "%s: features, bwd_streams, bwd16, relu_bits, g_acts, scratch must be 16-byte aligned", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const StashLayout L(B, V, N);
    float* const g0 = static_cast<float*>(scratch);
    MV_HIP(launch_zero(d_points, (size_t)L.total * 3 * sizeof(float), st), who);
    MV_HIP(launch_zero(d_dirs, (size_t)L.total * 3 * sizeof(float), st), who);
    MV_HIP(launch_trunk_vjp_bf16(bwd16, relu_bits, g_acts, B, V, L.total, L.n_tiles, g0, st), who);
    FieldParams p = {};
    p.rays_o = points; p.rays_d = dirs; p.z = nullptr; p.images = images; p.features = features;
    p.k4 = intrinsics; p.einv = extrinsics_inv;
    p.B = B; p.V = V; p.R = N; p.S = 1; p.H = H; p.W = W; p.total = L.total; p.n_tiles = L.n_tiles;
    MV_HIP(launch_field_dz(p, g0, bwd_streams + (size_t)12 * kHiddenWFloats, nullptr, d_points, d_dirs, nullptr, st), who);
    return 0;
}

int mvnerf_stash_fused_acts(const float* stash, int B, int V, int N, float* acts, mvnerf_stream_t stream) {
    if (!stash || !acts) return fail(MVNERF_E_ARG, "mvnerf_stash_fused_acts: null pointer");
    if (B <= 0 || V <= 0 || N <= 0) return fail(MVNERF_E_ARG, "mvnerf_stash_fused_acts: B=%d V=%d N=%d", B, V, N);
    if (!aligned16(stash) || !aligned16(acts)) return fail(MVNERF_E_ALIGN, "mvnerf_stash_fused_acts: stash, acts must be 16-byte aligned");
    const StashLayout L(B, V, N);
    // fused slots 0, 2, 4, 6 = view mean, u1, u2, u3 (the odd ones are the blocks' hidden pre-activations)
    return hip_status(mvnerf::launch_tl_to_rows(stash + L.fused_slot(0), 2 * L.fused_stride(), 4, L.total, L.n_tiles, acts,
                                                static_cast<hipStream_t>(stream)),
                      "mvnerf_stash_fused_acts");
}

int mvnerf_adam_clip(float* param, const float* grad, float* m, float* v, long n, float lr_t, float beta1, float beta2,
                     float eps, float clip, const unsigned char* update_mask, mvnerf_stream_t stream) {
    if (!param || !grad || !m || !v) return fail(MVNERF_E_ARG, "mvnerf_adam_clip: null pointer");
    if (n <= 0) return fail(MVNERF_E_ARG, "mvnerf_adam_clip: n=%ld", n);
    return hip_status(mvnerf::launch_adam_clip(param, grad, m, v, n, lr_t, beta1, beta2, eps, clip, update_mask,
                                               static_cast<hipStream_t>(stream)),
                      "mvnerf_adam_clip");
}

size_t mvnerf_field_workspace_bytes(int B, int V, int R) {
    if (B <= 0 || V <= 0 || R <= 0) return 0;
    return (size_t)B * V * R * 128 * sizeof(float);
}

size_t mvnerf_render_workspace_bytes(int B, int V, int R, int S) {
    if (B <= 0 || V <= 0 || R <= 0 || S <= 0) return 0;
    return carve(nullptr, (long)B * R, V, S).bytes;
}

// mvnerf_render_fwd and mvnerf_render_fwd_split: the same two-pass composition; `split` says which field kernel runs the passes
static int render_fwd(const char* who, bool split, const float* rays_o, const float* rays_d, const float* images, const float* features,
                      const float* intrinsics, const float* extrinsics_inv, const float* packed_coarse, const float* packed_fine,
                      const void* split_coarse, const void* split_fine, const float* u_coarse, const float* u_fine, int B, int V, int R,
                      int S, int H, int W, double near_, double far_, int q7_mode, float* rgb, float* depth, float* fine_rgb,
                      float* fine_depth, void* workspace, float* texel_tables, int tables_ready, mvnerf_stream_t stream, int which = -1,
                      float* range_status = nullptr) {
    if (const int rc = split_choice_check(who, which)) return rc;
    if (!u_coarse || !u_fine || !rgb || !depth || !fine_rgb || !fine_depth || !workspace || !packed_fine ||
        (split && (!split_coarse || !split_fine)))
        return fail(MVNERF_E_ARG, "%s: null pointer", who);
    if (S != 64) return fail(MVNERF_E_SHAPE, "%s: S=%d, only the reference's n_samples=64 is built", who, S);
    if (B <= 0 || R <= 0) return fail(MVNERF_E_ARG, "%s: B=%d R=%d", who, B, R);
    if (!aligned16(workspace)) return fail(MVNERF_E_ALIGN, "%s: workspace must be 16-byte aligned", who);
    if (const int rc = range_status_check(who, range_status)) return rc;
    const long n_rays = (long)B * R;
    if (n_rays * 2 * S >= (1L << 31)) return fail(MVNERF_E_SHAPE, "%s: B*R*2S too large", who);
    const Workspace w = carve(workspace, n_rays, V, S);
    int rc;
    const float *table_c = nullptr, *table_f = nullptr;
    if (texel_tables) {                                       // [coarse net | fine net], mvnerf_texel_table_bytes each
        float* tf = texel_tables + mvnerf_texel_table_bytes(B, V, H, W) / sizeof(float);
        if (!tables_ready) {
            if ((rc = mvnerf_project_texels2(features, packed_coarse, packed_fine, B, V, H, W, texel_tables, tf, stream))) return rc;
        }
        table_c = texel_tables;
        table_f = tf;
    }
    const char* field_who = split ? "mvnerf_field_eval_split" : "mvnerf_field_eval";
    const FieldKind kind = {split ? kFieldSplit : kFieldFp32, false, MVNERF_E_SHAPE};
    const FieldArgs coarse = {rays_o, rays_d, w.z, images, features, table_c, intrinsics, extrinsics_inv, packed_coarse, split_coarse, B, V, R, S,
                              H, W, w.rgbs_c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, w.dir_bias};
    const FieldArgs fine = {rays_o, rays_d, w.z_all, images, features, table_f, intrinsics, extrinsics_inv, packed_fine, split_fine, B, V, R,
                            2 * S, H, W, w.rgbs_f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, w.dir_bias};
    if ((rc = mvnerf_stratified_depths(u_coarse, (int)n_rays, S, near_, far_, w.z, stream))) return rc;
    if ((rc = field_pass(field_who, coarse, kind, stream, which, range_status))) return rc;
    if ((rc = mvnerf_composite(w.z, w.rgbs_c, (int)n_rays, S, rgb, depth, w.weights, stream))) return rc;
    if ((rc = mvnerf_resample(w.z, w.weights, u_fine, (int)n_rays, S, q7_mode, w.z_all, nullptr, nullptr, nullptr, nullptr, stream)))
        return rc;
    if ((rc = field_pass(field_who, fine, kind, stream, which, range_status ? range_status + 1 : nullptr))) return rc;
    return mvnerf_composite(w.z_all, w.rgbs_f, (int)n_rays, 2 * S, fine_rgb, fine_depth, nullptr, stream);
}

int mvnerf_render_fwd(const float* rays_o, const float* rays_d, const float* images, const float* features,
                      const float* intrinsics, const float* extrinsics_inv, const float* packed_coarse,
                      const float* packed_fine, const float* u_coarse, const float* u_fine, int B, int V, int R,
                      int S, int H, int W, double near_, double far_, int q7_mode, float* rgb, float* depth,
                      float* fine_rgb, float* fine_depth, void* workspace, float* texel_tables, int tables_ready,
                      mvnerf_stream_t stream) {
    return render_fwd("mvnerf_render_fwd", false, rays_o, rays_d, images, features, intrinsics, extrinsics_inv, packed_coarse, packed_fine,
                      nullptr, nullptr, u_coarse, u_fine, B, V, R, S, H, W, near_, far_, q7_mode, rgb, depth, fine_rgb, fine_depth, workspace,
                      texel_tables, tables_ready, stream);
}

int mvnerf_render_fwd_split(const float* rays_o, const float* rays_d, const float* images, const float* features,
                            const float* intrinsics, const float* extrinsics_inv, const float* packed_coarse,
                            const float* packed_fine, const void* split_coarse, const void* split_fine, const float* u_coarse,
                            const float* u_fine, int B, int V, int R, int S, int H, int W, double near_, double far_, int q7_mode,
                            float* rgb, float* depth, float* fine_rgb, float* fine_depth, void* workspace, float* texel_tables,
                            int tables_ready, mvnerf_stream_t stream) {
    return render_fwd("mvnerf_render_fwd_split", true, rays_o, rays_d, images, features, intrinsics, extrinsics_inv, packed_coarse,
                      packed_fine, split_coarse, split_fine, u_coarse, u_fine, B, V, R, S, H, W, near_, far_, q7_mode, rgb, depth, fine_rgb,
                      fine_depth, workspace, texel_tables, tables_ready, stream);
}

int mvnerf_render_fwd_split_ex(const float* rays_o, const float* rays_d, const float* images, const float* features,
                               const float* intrinsics, const float* extrinsics_inv, const float* packed_coarse,
                               const float* packed_fine, const void* split_coarse, const void* split_fine, const float* u_coarse,
                               const float* u_fine, int B, int V, int R, int S, int H, int W, double near_, double far_, int q7_mode,
                               float* rgb, float* depth, float* fine_rgb, float* fine_depth, void* workspace, float* texel_tables,
                               int tables_ready, int which, float* range_status, mvnerf_stream_t stream) {
    return render_fwd("mvnerf_render_fwd_split_ex", true, rays_o, rays_d, images, features, intrinsics, extrinsics_inv, packed_coarse,
                      packed_fine, split_coarse, split_fine, u_coarse, u_fine, B, V, R, S, H, W, near_, far_, q7_mode, rgb, depth, fine_rgb,
                      fine_depth, workspace, texel_tables, tables_ready, stream, which, range_status);
}

}  // extern "C"
