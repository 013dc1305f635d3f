// Host side of the extern "C" layer, shared by every translation unit that defines entry points: alignment predicates, the HIP
// error -> return code rule, the early-return macros, the workspace allocator, the stash format, and the frozen-trunk stage of the
// two pose-driven composite calls.  Nothing in here is seen by device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mvnerf_hip.h"
#include "mvnerf_kernels.h"

namespace mvnerf {

// (NULL counts as aligned: optional pointers are checked when given)
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool aligned256(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 255u) == 0; }

// 0, or the HIP error code (> 0) with "<who>: <HIP's text>" as the message of mvnerf_last_error()
inline int hip_status(hipError_t e, const char* who) {
    return e == hipSuccess ? 0 : api_fail((int)e, "%s: %s", who, hipGetErrorString(e));
}

// return the first non-zero return code / HIP error of an entry point's steps
#define MV_RC(x)                  \
    do {                          \
        int rc_ = (x);            \
        if (rc_ != 0) return rc_; \
    } while (0)
#define MV_HIP(x, who) MV_RC(mvnerf::hip_status((x), who))

// Carves a caller-provided workspace front to back; every piece starts on a multiple of `align` bytes from the base (256 for the
// composite calls, whose base must be 256-byte aligned).  Carving at NULL gives the size: addresses are integers until they are handed out.
struct Bump {
    uintptr_t base;
    size_t used = 0, align;
    explicit Bump(void* base_, size_t align_ = 256) : base(reinterpret_cast<uintptr_t>(base_)), align(align_) {}
    void* take(size_t bytes) {
        void* q = reinterpret_cast<void*>(base + used);
        used += (bytes + align - 1) / align * align;
        return q;
    }
    float* floats(size_t n) { return static_cast<float*>(take(n * sizeof(float))); }
    size_t bytes() const { return used; }
};

// The stash of a training-mode field pass over B scenes of `rows` samples (R * S; N query points): pre-activations in tile layout
// [slot][tile][128][32], a tile being 32 consecutive samples.  7 per-view slots x0,h1,x1,h2,x2,h3,x3 (layer 0 and the three per-view
// blocks: block input, hidden; tile = view tile (b * V + v) * tiles_per_b + k) and behind them 7 fused slots mean,h4,x4,h5,x5,h6,x6
// (the view mean and the three fusion blocks; tile = b * tiles_per_b + k).  Offsets and strides are in floats.
struct StashLayout {
    static constexpr long kTileFloats = 128 * 32;
    static constexpr int kSlots = 7;                       // per-view, and fused
    long total, n_tiles, view_tiles;                       // samples, their 32-sample tiles, tiles of one per-view slot
    StashLayout(int B, int V, long rows) : total((long)B * rows), n_tiles((total + 31) / 32), view_tiles(n_tiles * V) {}
    long view_stride() const { return view_tiles * kTileFloats; }        // FieldParams::stash_stride
    long fused_stride() const { return n_tiles * kTileFloats; }          // FieldParams::stash_fused_stride
    size_t view_slot(int k) const { return (size_t)k * view_stride(); }
    size_t fused_slot(int m) const { return (size_t)kSlots * view_stride() + (size_t)m * fused_stride(); }
    size_t bytes() const { return fused_slot(kSlots) * sizeof(float); }
};

// ---- pose rows through the frozen trunk (mvnerf_grasp_* and mvnerf_language_loss_and_grads; defined in grasp_api.hip) ----------------
// Rows of one scene as the trunk sees them: the multi-view kernels want whole 32-point tiles per scene.
inline long pose_rows_ld(int V, long n) { return V > 1 ? (n + 31) / 32 * 32 : n; }
// rows n .. ld of every scene repeat row n - 1 (their cotangents and tangents stay zero); nothing to do when ld == n
int pad_pose_rows(const char* who, float* points, float* dirs, int B, long n, long ld, hipStream_t st);
// The trunk on B scenes of ld query rows (points, dirs (B, ld, 3); z (B, ld) zero: the points are the samples) with its pre-activations
// kept in `stash`, then the four fused activations as rows in `acts` (4, B * ld, 128).  rgbs (B, ld, 4) and field_ws are scratch.
inline int pose_rows_trunk(const float* points, const float* dirs, const float* z, const float* images, const float* features,
                           const float* intrinsics, const float* extrinsics_inv, const float* packed_net, const void* split, int B, int V,
                           long ld, int H, int W, float* rgbs, float* stash, void* field_ws, float* acts, mvnerf_stream_t stream) {
    MV_RC(mvnerf_field_eval_stash_split(points, dirs, z, images, features, nullptr, intrinsics, extrinsics_inv, packed_net, split, B, V, (int)ld,
                                        1, H, W, rgbs, stash, field_ws, stream));
    return mvnerf_stash_fused_acts(stash, B, V, (int)ld, acts, stream);
}

// ---- the LanguageNeRF step and its optimiser (language_api.hip, language_opt.hip) ----------------------------------------------------
// every check of mvnerf_language_loss_and_grads on its struct, without a launch: 0 or its return code with the message set
int language_validate(const mvnerf_language_call* call);

}  // namespace mvnerf
