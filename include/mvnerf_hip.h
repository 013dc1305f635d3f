/* mvnerf_hip.h - C ABI of libmvnerf_hip.so: the MI355X (gfx950) implementation of the volumetric
 * rendering hot path of TWeber132/thesis-clip-nerf (src/lib/mvnerf).
 *
 * The reference has no FFI on this path: it is Python calling TensorFlow ops.  Each entry point
 * below therefore names the reference Python function it replaces (file:line under
 * /root/reference/src/lib); INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32/int32 unless marked [host]; tensors are dense,
 *    row-major, in the shapes the reference uses (B scenes, V source views, R rays, S samples);
 *  - the caller owns every buffer; nothing is allocated, freed or retained by the library;
 *  - `stream` is a hipStream_t (NULL = default stream); all work is stream-ordered and asynchronous;
 *  - return value 0 = success; < 0 = argument error (MVNERF_E_*); > 0 = hipError_t of a failed
 *    launch.  mvnerf_last_error() returns a thread-local description of the last failure.
 */
#ifndef MVNERF_HIP_H
#define MVNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mvnerf_stream_t; /* hipStream_t */

#define MVNERF_NET_PARAMS 247300   /* floats of one MLP in Keras order, see mvnerf_pack_net */
#define MVNERF_N_FEATURES 256
#define MVNERF_HIDDEN 128

#define MVNERF_E_ARG (-1)          /* null pointer / non-positive size */
#define MVNERF_E_SHAPE (-2)        /* unsupported shape (message says which) */
#define MVNERF_E_ALIGN (-3)        /* pointer not 16-byte aligned where required */

#define MVNERF_Q7_ZERO 0           /* sample_pdf: out-of-range gather yields 0 (TF-GPU gather_nd) */
#define MVNERF_Q7_CLAMP 1          /* sample_pdf: clamp `above` to the last bin */

int mvnerf_abi_version(void);
const char* mvnerf_last_error(void);

/* Number of floats of the MFMA-ordered weight image produced by mvnerf_pack_net. */
size_t mvnerf_packed_net_floats(void);

/* Re-lay one MLP (MVResNetMLPNeRFEmbedding + RenderReadout, layers.py:334-397) from Keras order
 *   W0[379,128] b0[128] | 6 x (W1[128,128] b1[128] W2[128,128] b2[128]) | Wr[128,4] br[4]
 * (kernel[in,out], bias[out]; 247300 floats) into the operand order the MFMA kernel streams.
 * Call once per weight update.  `packed` must be 16-byte aligned. */
int mvnerf_pack_net(const float* net_keras, float* packed, mvnerf_stream_t stream);

/* get_specific_rays / get_rays (nerf_utils.py:15-35).  d = normalize(M * [u, v, 1]) in float64,
 * rounded to fp32 on store; o = origin.  M = E[:3,:3] @ inv(K[:3,:3]) and origin = E[:3,3] are
 * [host] float64 (the 3x3 inverse stays in NumPy/LAPACK on the host, as in the reference).
 * If u and v are NULL the full image grid is generated: ray n = (v = n / width, u = n % width)
 * for n < width*height (get_rays); otherwise n_rays pixels (u[n], v[n]) (get_specific_rays).
 * rays_o, rays_d: (n_rays,3) fp32.  rays_d64 (optional, may be NULL): (n_rays,3) float64. */
int mvnerf_get_rays(const double* m3x3_host, const double* origin_host, const float* u, const float* v,
                    int n_rays, int width, int normalize, float* rays_o, float* rays_d, double* rays_d64,
                    mvnerf_stream_t stream);

/* sample_along_ray depths (nerf_utils.py:49-58): z[n,i] = fl32(near + i*step) + u[n,i]*fl32(step),
 * step = (far-near)/n_samples in float64.  u, z: (n_rays, n_samples). */
int mvnerf_stratified_depths(const float* u, int n_rays, int n_samples, double near_, double far_,
                             float* z, mvnerf_stream_t stream);

/* One evaluation pass of the radiance field (model_v0.py:122-144 coarse, :157-180 fine):
 *   p = o + z*d                              (nerf_utils.py:59-60 / model_v0.py:157-158)
 *   per view: cam = Einv*[p;1], pix = K4*cam (compute_pixel_in_image_mv, nerf_utils.py:64-81)
 *             bilinear gather of [2*img-1 | features] at pix (get_projection_features_mv,
 *             nerf_utils.py:277-285 -> tensorflow_addons interpolate_bilinear, indexing='xy')
 *             cam_dir = Einv*[d;1]           (world_to_camera_direction_vector_mv, :84-105)
 *             PE(cam xyz), PE(cam_dir)       (position_encoding, nerf_utils.py:108-126)
 *             Dense 379->128 + 3 ResNet blocks                       (layers.py:354-366)
 *   mean over views, 3 ResNet blocks         (layers.py:368-374)
 *   Dense 128->4, sigmoid / softplus         (RenderReadout, layers.py:392-397)
 * rays_o, rays_d (B,R,3); z (B,R,S); images (B,V,H,W,3) in [0,1]; features (B,V,H,W,256), 16-byte
 * aligned; intrinsics, extrinsics_inv (B,V,4,4); packed_net from mvnerf_pack_net.
 * rgbs (B,R,S,4) = (r,g,b,sigma) per sample, 16-byte aligned.
 * tap_idx (optional, may be NULL): (B,V,R,S,4) int32 linear texel indices
 * (b*V+v)*H*W + y*W + x of the tl,tr,bl,br taps (the integer contract of a6).
 * pix (optional, may be NULL): (B,V,R,S,2) fp32 pixel locations (x,y).
 * embedding (optional, may be NULL): (B,R,S,128) output of MVResNetMLPNeRFEmbedding (layers.py:379),
 * 16-byte aligned.
 * acts_per_view (optional): (4, B*V, R, S, 128) and acts_fused (optional): (4, B, R, S, 128): the eight
 * activations the trunk returns with complete_output=True (layers.py:364-377): [x0, f1, f2, f3] per view and
 * [mean, u1, u2, u3] after the view mean; this is what LanguageNeRF consumes (lmvnerf/model_v4.py:261-262).
 * Arbitrary query points (not on rays): pass the points as rays_o, their directions as rays_d, z = 0, S = 1.
 * workspace: 16-byte aligned device scratch of mvnerf_field_workspace_bytes(B,V,R) bytes. */
int mvnerf_field_eval(const float* rays_o, const float* rays_d, const float* z, const float* images,
                      const float* features, const float* intrinsics, const float* extrinsics_inv,
                      const float* packed_net, int B, int V, int R, int S, int H, int W, float* rgbs,
                      int32_t* tap_idx, float* pix, float* embedding, float* acts_per_view, float* acts_fused,
                      void* workspace, mvnerf_stream_t stream);

/* Bytes of scratch mvnerf_field_eval needs (B*V*R*128 floats: the per-(view, ray) part of layer 0). */
size_t mvnerf_field_workspace_bytes(int B, int V, int R);

/* ---- Texel table: the feature part of layer 0 hoisted from samples to texels. ----
 * The first Dense of MVResNetMLPNerfEmbedding (layers.py:357-363) is linear in its input, and the gathered feature
 * vector (model_v0.py:131-136, tfa interpolate_bilinear) is linear in the four texels it blends, so
 *     W0[123:379]^T lerp(f_tl, f_tr, f_bl, f_br) == lerp(W0f^T f_tl, W0f^T f_tr, W0f^T f_bl, W0f^T f_br)
 * up to fp32 rounding (measured: tests/test_gpu_parity.py, same 1e-4 bar as the direct form).  The table holds
 * W0f^T f for every texel of every source view: (B*V,H,W,128) floats, features in accumulator order.  It depends
 * on the feature maps and on ONE net's W0 (coarse and fine nets need a table each); it pays off when a table is
 * used for more samples than it has texels (R*S >= H*W; rendering a frame chunk by chunk re-uses it).
 * mvnerf_field_eval_table == mvnerf_field_eval with 128 of the 190 layer-0 k-steps replaced by a 128-channel
 * lerp of table rows; every output, including tap_idx / pix / the activation taps, has the same meaning. */
size_t mvnerf_texel_table_bytes(int B, int V, int H, int W);
int mvnerf_project_texels(const float* features, const float* packed_net, int B, int V, int H, int W, float* texel_table,
                          mvnerf_stream_t stream);
/* Two nets (coarse, fine) from ONE read of the feature maps; packed_net_b / texel_table_b may both be NULL. */
int mvnerf_project_texels2(const float* features, const float* packed_net, const float* packed_net_b, int B, int V, int H, int W,
                           float* texel_table, float* texel_table_b, mvnerf_stream_t stream);
int mvnerf_field_eval_table(const float* rays_o, const float* rays_d, const float* z, const float* images,
                            const float* features, const float* texel_table, const float* intrinsics,
                            const float* extrinsics_inv, const float* packed_net, int B, int V, int R, int S, int H, int W,
                            float* rgbs, int32_t* tap_idx, float* pix, float* embedding, float* acts_per_view,
                            float* acts_fused, void* workspace, mvnerf_stream_t stream);

/* ---- bf16 variant of the field pass (BASELINE.json configs 3 and 5: bf16 weights and MFMA inputs, fp32
 * accumulate, fp32 geometry / biases / read-out activations).  Not held to the 1e-4 fp32 bar; the achieved error
 * against the fp32 oracle is stated in DESIGN.md and tests/test_gpu_bf16.py. ---- */
size_t mvnerf_packed_net_bf16_bytes(void);
/* Keras-order fp32 MLP (see mvnerf_pack_net) -> bf16 MFMA operand stream.  packed16: 16-byte aligned. */
int mvnerf_pack_net_bf16(const float* net_keras, void* packed16, mvnerf_stream_t stream);
/* mvnerf_project_texels on the bf16 MFMA: features and W0's feature rows rounded to bf16, fp32 accumulation, fp32 table
 * (same layout) - for mvnerf_field_eval_bf16(texel_table = ...); 16x less matrix time than the fp32 projection. */
int mvnerf_project_texels_bf16(const float* features, const void* packed16, const void* packed16_b, int B, int V, int H, int W,
                               float* texel_table, float* texel_table_b, mvnerf_stream_t stream);   /* _b: optional second net */
/* As mvnerf_field_eval, with the Dense kernels taken from packed16 (biases and the per-ray layer-0 seed still come
 * from the fp32 image packed_net).  Optional outputs: tap_idx, embedding, acts_fused (4,B,R,S,128) = the view mean and
 * the three fusion blocks (the part of complete_output that LanguageNeRF consumes, lmvnerf/model_v4.py:261).
 * texel_table (optional, may be NULL): mvnerf_project_texels(features, packed_net) - the fp32 table of the same net;
 * the feature rows of layer 0 are then an fp32 lerp of table rows instead of bf16 MFMA products. */
int mvnerf_field_eval_bf16(const float* rays_o, const float* rays_d, const float* z, const float* images,
                           const float* features, const float* texel_table, const float* intrinsics, const float* extrinsics_inv,
                           const float* packed_net, const void* packed16, int B, int V, int R, int S, int H, int W,
                           float* rgbs, int32_t* tap_idx, float* embedding, float* acts_fused, void* workspace,
                           mvnerf_stream_t stream);

/* The two entry points above with the source feature maps STORED as bf16 (B,V,H,W,256) NHWC - BASELINE.json config 5 as SURVEY.md 8d
 * states it ("feature map + weights bf16"): 512-byte texel rows, what encoders.FeatureProducer(out_dtype=torch.bfloat16) emits.  The
 * bilinear gather of get_projection_features_mv (nerf_utils.py:277-285) widens the taps to fp32 (exact), lerps in fp32 and rounds once, as
 * with fp32 maps - so on maps whose fp32 values are bf16-representable the results are bit-identical to the fp32-map entry points;
 * the projection / gather reads half the bytes.  Source images stay fp32. */
int mvnerf_project_texels_bf16maps(const void* features_bf16, const void* packed16, const void* packed16_b, int B, int V, int H, int W,
                                   float* texel_table, float* texel_table_b, mvnerf_stream_t stream);
int mvnerf_field_eval_bf16maps(const float* rays_o, const float* rays_d, const float* z, const float* images,
                               const void* features_bf16, const float* texel_table, const float* intrinsics, const float* extrinsics_inv,
                               const float* packed_net, const void* packed16, int B, int V, int R, int S, int H, int W,
                               float* rgbs, int32_t* tap_idx, float* embedding, float* acts_fused, void* workspace,
                               mvnerf_stream_t stream);

/* ---- fp32-grade field pass on the 16-bit matrix pipe ("split"): every fp32 GEMM operand is represented by 16-bit pieces and a
 * product block is issued as a few 16-bit MFMAs with fp32 accumulation.  Same function, inputs, outputs and 1e-4 bar as
 * mvnerf_field_eval / mvnerf_field_eval_table (model_v0.py:122-144 / :157-180).  Three kernels read the same packed_split image
 * (mvnerf_set_split_kernel):
 *   MVNERF_SPLIT_F16X3 (default)  two fp16 pieces per operand (round-to-nearest twice, the remainder scaled by 64: 22-24 significant
 *                                 bits), three v_mfma_f32_16x16x32_f16 per block; per ResNet block as close to a float64 evaluation as
 *                                 the fp32 MFMA (tests/test_gpu_split.py); range |w| < 1023, |activation| < 4.19e6
 *                                 (MVNERF_F16X3_MAX_WEIGHT / _MAX_ACT below; csrc/field_eval_split16_impl.h, field_eval_split16h.hip)
 *   MVNERF_SPLIT_BF16X6           three bf16 pieces per operand, an EXACT cut, the six products of order >= 2^-16 as
 *                                 v_mfma_f32_16x16x32_bf16; dropped terms <= 2^-24 relative; full fp32 range (field_eval_split16.hip)
 *   MVNERF_SPLIT_BF16X6_32        the same products as v_mfma_f32_32x32x16_bf16 (round 2's kernel, field_eval_split.hip)
 * The training forward (mvnerf_field_eval_stash_split) follows the same choice (the 32x32x16 kernel has no fp16 form); the backward's layer
 * launches always use fp16 two-piece products with a per-tensor power-of-two scale on the gradients (csrc/train_ops.hip, MVT_BWD_F16). ---- */
#define MVNERF_SPLIT_F16X3 0
#define MVNERF_SPLIT_BF16X6 1
#define MVNERF_SPLIT_BF16X6_32 2
/* Range of MVNERF_SPLIT_F16X3.  Its weight pieces are rn16(64 w), its activation pieces rn16(v / 64), and fp16 rounds to infinity from
 * 65520 upward: the kernel is correct for |w| < 1023.75 and |v| < 4193280 and silently wrong beyond (inf - inf inside the products; a
 * relu can turn the NaN into 0, so the output need not show it).  The two constants are those thresholds, slightly conservative.
 * Weights: mvnerf_net_range.  Activations: the range status of the _ex entry points.  Out of range, run MVNERF_SPLIT_BF16X6 (same
 * packed_split image, full fp32 range).
 * The training BACKWARD is tighter: its weight-gradient GEMM cuts relu(stashed pre-activation) as rn16(64 a), so every stashed
 * pre-activation has to stay below MVNERF_F16X3_MAX_WEIGHT as well - 4096 times less than the forward allows.  That limit is detected
 * (range status of mvnerf_field_eval_stash_split_ex against MVNERF_F16X3_MAX_WEIGHT), not lifted. */
#define MVNERF_F16X3_MAX_WEIGHT 1023.0f
#define MVNERF_F16X3_MAX_ACT 4.19e6f
/* Process-wide choice of the kernel behind mvnerf_field_eval_split / mvnerf_render_fwd_split; returns the previous value (< 0 and
 * no change for an unknown value).  The environment variable MVNERF_SPLIT_MFMA ("f16x3" | "bf16x6" | "32x32x16"), read at every
 * launch, overrides it (A/B runs, tests). */
int mvnerf_set_split_kernel(int which);
size_t mvnerf_packed_net_split_bytes(void);
/* Keras-order fp32 MLP (see mvnerf_pack_net) -> the operand streams of the three kernels above.  packed_split: 16-byte aligned. */
int mvnerf_pack_net_split(const float* net_keras, void* packed_split, mvnerf_stream_t stream);
/* As mvnerf_field_eval (texel_table NULL) / mvnerf_field_eval_table, with the Dense kernels taken from packed_split
 * (biases, the per-ray layer-0 seed and the texel table still come from the fp32 image packed_net).  Optional outputs
 * as there: tap_idx, pix, embedding, acts_per_view, acts_fused. */
int mvnerf_field_eval_split(const float* rays_o, const float* rays_d, const float* z, const float* images,
                            const float* features, const float* texel_table, const float* intrinsics, const float* extrinsics_inv,
                            const float* packed_net, const void* packed_split, int B, int V, int R, int S, int H, int W,
                            float* rgbs, int32_t* tap_idx, float* pix, float* embedding, float* acts_per_view, float* acts_fused,
                            void* workspace, mvnerf_stream_t stream);
/* mvnerf_field_eval_split with the kernel chosen for THIS call and an optional range status.
 * which: -1 = the process-wide value (mvnerf_set_split_kernel), or MVNERF_SPLIT_F16X3 / _BF16X6 / _BF16X6_32 for this call only; any
 *   other value is MVNERF_E_ARG.  MVNERF_SPLIT_MFMA in the environment still overrides both.
 * range_status (optional, may be NULL): ONE device float, 4-byte aligned (else MVNERF_E_ALIGN).  When the f16x3 kernel runs the pass, its
 *   range-guarded copy runs instead (csrc/field_eval_split16h_guard.hip; bit-identical results) and max-accumulates into it the largest
 *   |v| of every value it cuts into fp16 activation pieces: the PE / rgb operands, the gathered features (direct form), and relu(x),
 *   relu(h) in front of every hidden Dense layer, per view and fused (after the relu).  Compare with MVNERF_F16X3_MAX_ACT.  The caller
 *   zeroes it; calls accumulate (the chunks of a frame).  It is the bit pattern of a non-negative float under an unsigned max: a NaN operand
 *   leaves a NaN, infinity leaves infinity.  The other two kernels have the full fp32 range and leave it untouched.  Nothing is read back:
 *   reading the status is the caller's synchronisation. */
int mvnerf_field_eval_split_ex(const float* rays_o, const float* rays_d, const float* z, const float* images,
                               const float* features, const float* texel_table, const float* intrinsics, const float* extrinsics_inv,
                               const float* packed_net, const void* packed_split, int B, int V, int R, int S, int H, int W,
                               float* rgbs, int32_t* tap_idx, float* pix, float* embedding, float* acts_per_view, float* acts_fused,
                               void* workspace, int which, float* range_status, mvnerf_stream_t stream);
/* Weight range of a Keras-order net (247300 floats, see mvnerf_pack_net), two device floats, same bit-pattern convention (NaN stays NaN):
 * out2[0] = max |w| over what mvnerf_pack_net_split cuts into 16-bit pieces (the 379 rows of W0 and the 12 hidden kernels; no bias, no
 * read-out) - compare with MVNERF_F16X3_MAX_WEIGHT;  out2[1] = max |.| over all variables.  out2: 4-byte aligned; overwritten. */
int mvnerf_net_range(const float* net_keras, float* out2, mvnerf_stream_t stream);

/* MVVNeRFRenderer.volumetric_render (model_v0.py:89-100) with sigma_to_alpha (nerf_utils.py:129-140).
 * z (n_rays,S); rgbs (n_rays,S,4); S in {64,128,192,256}.
 * rgb (n_rays,3); depth (n_rays); weights (optional, may be NULL) (n_rays,S). */
int mvnerf_composite(const float* z, const float* rgbs, int n_rays, int S, float* rgb, float* depth,
                     float* weights, mvnerf_stream_t stream);

/* Hierarchical resampling (model_v0.py:150-156): z_mid, probs = w[1:-1], sample_pdf
 * (nerf_utils.py:143-176) with explicit uniforms u_fine, concat, ascending sort.
 * z, weights, u_fine: (n_rays,64).  z_all: (n_rays,128).  Optional outputs (may be NULL):
 * z_fine (n_rays,64) fp32, above / below (n_rays,64) int32 (the integer contract of a13),
 * fine_rank (n_rays,64) int32: position of importance sample i inside z_all (the sort permutation, kept for
 * the backward pass). */
int mvnerf_resample(const float* z, const float* weights, const float* u_fine, int n_rays, int S,
                    int q7_mode, float* z_all, float* z_fine, int32_t* above, int32_t* below, int32_t* fine_rank,
                    mvnerf_stream_t stream);

/* ---- op-level (unfused) entry points: one per reference function, same scalar code as the fused
 * kernels; used by the op-level parity tests and by callers that want a single operator. ---- */

/* world = o + z*d (nerf_utils.py:59-60).  o,d (n_rays,3); z (n_rays,S) -> world (n_rays,S,3). */
int mvnerf_points_on_rays(const float* rays_o, const float* rays_d, const float* z, int n_rays, int S, float* world,
                          mvnerf_stream_t stream);

/* compute_pixel_in_image_mv (nerf_utils.py:64-81).  world (B,N,3); intrinsics, extrinsics_inv (B,V,4,4)
 * -> pixel_locations (B,V,N,2) [x,y], camera_points_homogeneous (B,V,N,4). */
int mvnerf_project_points(const float* world, const float* intrinsics, const float* extrinsics_inv, int B, int V,
                          int N, float* pixel_locations, float* camera_points, mvnerf_stream_t stream);

/* world_to_camera_direction_vector_mv (nerf_utils.py:84-105; homogeneous w = 1).
 * dirs (B,R,3); extrinsics_inv (B,V,4,4) -> (B,V,R,3). */
int mvnerf_camera_directions(const float* dirs, const float* extrinsics_inv, int B, int V, int R, float* out,
                             mvnerf_stream_t stream);

/* position_encoding (nerf_utils.py:108-126).  x: n_elems scalars (any (...,D) flattened);
 * out: n_elems * 2 * n_freq, layout per element [k][sin,cos] (=> (..., D*2*n_freq) as (d n f)). */
int mvnerf_position_encoding(const float* x, long n_elems, int n_freq, float pos_encoding_freq, float* out,
                             mvnerf_stream_t stream);

/* get_projection_features_mv (nerf_utils.py:277-285): tensorflow_addons interpolate_bilinear
 * (indexing='xy') of the grid [images | features].  images (BV,H,W,3) as given (the caller normalises),
 * features (BV,H,W,256), pixel_locations (BV,Q,2) -> out (BV,Q,259); tap_idx (optional) (BV,Q,4) int32. */
int mvnerf_bilinear_gather(const float* images, const float* features, const float* pixel_locations, int BV, int Q,
                           int H, int W, float* out, int32_t* tap_idx, mvnerf_stream_t stream);

/* sigma_to_alpha (nerf_utils.py:129-140), elementwise over n values. */
int mvnerf_sigma_to_alpha(const float* sigma, const float* dists, long n, float* alpha, mvnerf_stream_t stream);

/* sample_pdf (nerf_utils.py:143-176) with explicit uniforms.  bins (n_rays,63); weights (n_rays,62);
 * u (n_rays,64) -> samples (n_rays,64); above / below (optional) (n_rays,64) int32. */
int mvnerf_sample_pdf(const float* bins, const float* weights, const float* u, int n_rays, int n_bins, int n_samples,
                      int q7_mode, float* samples, int32_t* above, int32_t* below, mvnerf_stream_t stream);

/* RenderReadout (layers.py:392-397).  embedding (n,128); wr kernel[128,4], br bias[4] (Keras layout)
 * -> rgbs (n,4) = (sigmoid rgb, softplus sigma). */
int mvnerf_readout(const float* embedding, const float* wr, const float* br, long n, float* rgbs,
                   mvnerf_stream_t stream);

/* render_view epilogue (model_v0.py:275-281).  rgb (n,3), depth (n) -> rgb8 (n,3) = uint8(clip(rgb*255,0,255)),
 * depth8 (n) = uint8(255*(depth-min)/(max-min)).  minmax_scratch: 2 floats of device scratch. */
int mvnerf_finish_view(const float* rgb, const float* depth, long n, float* minmax_scratch, uint8_t* rgb8,
                       uint8_t* depth8, mvnerf_stream_t stream);

/* ---- training step (MVVNeRFRenderer.train_step, model_v0.py:186-197; optimize, nerf_utils.py:8-12) ----
 * Gradients of every MLP variable, including the path through the importance samples that the reference leaves
 * open (no stop_gradient).  V > 1 needs R*S to be a multiple of 32. */

/* Bytes of the activation stash of one mvnerf_field_eval_stash call: 7 per-view + 7 fused pre-activation tensors in tile layout
 * (per view x0 h1 x1 h2 x2 h3 x3, then mean h4 x4 h5 x5 h6 x6).  The per-view slot of x3 is part of the layout but is not written:
 * nothing reads it (the backward of the view mean needs no activation; for V = 1 it is the fused slot of the mean). */
size_t mvnerf_stash_bytes(int B, int V, int R, int S);
/* Weight-gradient reduction of mvnerf_field_backward: every workgroup stores its partial of a layer's [dW | db] span and the partials
 * are summed in workgroup order - bit-identical gradients for identical inputs.  Until the middle of round 2 this was a mode (0 =
 * fp32 atomics, 1 = stored partials); with the partials added by a parallel fixed-order reduction it is also the faster of the two
 * and the only one.  The switch is kept for its callers: it records the flag and returns the previous value, nothing else.  The
 * gradients w.r.t. sample depths (V > 1), ray origins / directions and the source feature maps still accumulate with atomics. */
int mvnerf_set_deterministic(int on);
/* Bytes of scratch mvnerf_field_backward needs (three gradient tensors in tile layout, the read-out's cotangent tile, the per-workgroup
 * weight-gradient partials and 14 x 64 floats of max |g| slots: the power-of-two scales of the layer launches' fp16 products). */
size_t mvnerf_field_backward_scratch_bytes(int B, int V, int R, int S);

/* mvnerf_field_eval in training mode: also stores the trunk's pre-activations into `stash`.
 * texel_table (optional, may be NULL): as in mvnerf_field_eval_table, for the forward value only - the backward
 * recomputes layer 0's inputs from the raw features either way. */
int mvnerf_field_eval_stash(const float* rays_o, const float* rays_d, const float* z, const float* images,
                            const float* features, const float* texel_table, const float* intrinsics,
                            const float* extrinsics_inv, const float* packed_net, int B, int V, int R, int S, int H, int W,
                            float* rgbs, float* stash, void* workspace, mvnerf_stream_t stream);
/* mvnerf_field_eval_stash with the Dense layers as split-bf16 MFMA products (mvnerf_field_eval_split): same stash layout,
 * consumed by the same mvnerf_field_backward. */
int mvnerf_field_eval_stash_split(const float* rays_o, const float* rays_d, const float* z, const float* images,
                                  const float* features, const float* texel_table, const float* intrinsics,
                                  const float* extrinsics_inv, const float* packed_net, const void* packed_split, int B, int V, int R,
                                  int S, int H, int W, float* rgbs, float* stash, void* workspace, mvnerf_stream_t stream);
/* ... with `which` and `range_status` as in mvnerf_field_eval_split_ex.  The stash holds the very fp32 values that are cut, so the status is
 * max(relu(stash)) joined with the layer-0 operands.  For training compare it with MVNERF_F16X3_MAX_WEIGHT: the backward cuts
 * relu(pre-activation) as a weight-side operand (see the constants). */
int mvnerf_field_eval_stash_split_ex(const float* rays_o, const float* rays_d, const float* z, const float* images,
                                     const float* features, const float* texel_table, const float* intrinsics,
                                     const float* extrinsics_inv, const float* packed_net, const void* packed_split, int B, int V, int R,
                                     int S, int H, int W, float* rgbs, float* stash, void* workspace, int which, float* range_status,
                                     mvnerf_stream_t stream);

/* The 12 hidden Dense kernels of one MLP and the three 128-row slabs of the layer-0 kernel, transposed, in
 * weight-stream order (15 x 16384 floats), for the dX GEMMs of the backward pass.
 * net_keras: 247300 floats (see mvnerf_pack_net). */
int mvnerf_pack_bwd_streams(const float* net_keras, float* bwd_streams, mvnerf_stream_t stream);

/* d pred = 2 (pred - label) / n and *loss += mean((pred - label)^2) (Keras MeanSquaredError, model_v0.py:193). */
int mvnerf_mse_grad(const float* pred, const float* label, long n, float* d_pred, float* loss, mvnerf_stream_t stream);

/* volumetric_render backward (model_v0.py:89-100): d_rgb (n_rays,3), d_depth (optional, n_rays), d_weights
 * (optional, n_rays x S) -> d_rgbs (n_rays,S,4) = gradient w.r.t. the per-sample (r,g,b,sigma), and d_z
 * (optional, n_rays x S) = gradient w.r.t. the depths through the intervals and the depth output.  S in {64,128}. */
int mvnerf_composite_bwd(const float* z, const float* rgbs, const float* d_rgb, const float* d_depth,
                         const float* d_weights, int n_rays, int S, float* d_rgbs, float* d_z, mvnerf_stream_t stream);

/* Backward of mvnerf_resample w.r.t. the coarse weights: d_z_all (n_rays,128), fine_rank from the forward call
 * -> d_weights (n_rays,64).  (The coarse depths depend on no variable, so no d_z is returned.) */
int mvnerf_resample_bwd(const float* z, const float* weights, const float* u_fine, const int32_t* fine_rank,
                        const float* d_z_all, int n_rays, int S, int q7_mode, float* d_weights, mvnerf_stream_t stream);

/* Backward of one mvnerf_field_eval_stash call: accumulates dL/d(net variables) into `grad` (247300 floats, Keras
 * order, caller zeroes it) given d_rgbs (B,R,S,4).  Inputs as in the forward call, plus net_keras, the
 * transposed streams and the stash.
 * d_z (optional, may be NULL): (B,R,S), INCREMENTED by the gradient w.r.t. the sample depths through the sample
 * positions (positional encoding of the camera point and the bilinear lerp factors).
 * d_features (optional, may be NULL): (B,V,H,W,256), INCREMENTED by the gradient w.r.t. the source feature maps
 * (combined_features is produced by trainable encoders in the reference, train_nerf.py:27-32; this is what flows
 * back to them). */
int mvnerf_field_backward(const float* rays_o, const float* rays_d, const float* z, const float* images,
                          const float* features, const float* intrinsics, const float* extrinsics_inv,
                          const float* net_keras, const float* bwd_streams, const float* stash, const float* rgbs,
                          const float* d_rgbs, int B, int V, int R, int S, int H, int W, void* scratch, float* grad,
                          float* d_z, float* d_features, mvnerf_stream_t stream);
/* mvnerf_field_backward with the forward's texel table of the SAME net (mvnerf_project_texels; optional, may be NULL).  With it the
 * gradient through the sample positions (d_z) takes the feature rows' part from four table rows per sample instead of recomputing
 * W0 . g0 over the 256 feature channels (same result up to fp32 rounding).  texel_grad (optional scratch, (B,V,H,W,128) floats,
 * needs texel_table): when d_features is wanted, the samples' layer-0 cotangents are scattered onto this 128-channel table gradient
 * and W0 is applied once per texel (dL/df[texel] = W0[123:379] . dL/dT[texel]) - a third of the atomics of the direct scatter and
 * no 379 x 128 product per sample; without it d_features takes the direct path.
 * Reference: the same tape of MVVNeRFRenderer.train_step (model_v0.py:186-197); the table is this library's re-association of
 * layers.py:361-366 (see mvnerf_project_texels). */
int mvnerf_field_backward_table(const float* rays_o, const float* rays_d, const float* z, const float* images,
                                const float* features, const float* texel_table, float* texel_grad, const float* intrinsics,
                                const float* extrinsics_inv, const float* net_keras, const float* bwd_streams, const float* stash,
                                const float* rgbs, const float* d_rgbs, int B, int V, int R, int S, int H, int W, void* scratch,
                                float* grad, float* d_z, float* d_features, mvnerf_stream_t stream);

/* c (M,N) = a (M,K) . bt (N,K)^T in fp32 (fp32 MFMA, one wave per 32 x 64 output block; small outputs with a long K are split along K,
 * the splits' partials go to `scratch` and are added in split order: no atomics, bit-identical from run to run).
 * For the GraspReadout's Dense layers (delta_ngf/layers.py:8-42 as used by lmvnerf/model_v4.py:290-322), their input / weight gradients
 * and the derivatives of those - skinny products (64 x 128 outputs over K = 64 512 rows, 1536 x 128 over K = 2688) on which the library
 * GEMM runs a handful of workgroups.  M % 32 == 0, N % 64 == 0, K % 8 == 0, 16-byte aligned row-major buffers;
 * scratch: mvnerf_gemm_nt_scratch_bytes(M,N,K) bytes (0 for shapes that are not split: NULL allowed). */
size_t mvnerf_gemm_nt_scratch_bytes(int M, int N, int K);
int mvnerf_gemm_nt(const float* a, const float* bt, float* c, int M, int N, int K, void* scratch, mvnerf_stream_t stream);
/* The Dense layer itself, c = a bt^T + bias (bias: N floats, added after the products - the result equals mvnerf_gemm_nt followed by a
 * broadcast add, bit for bit, in one launch less). */
int mvnerf_gemm_nt_bias(const float* a, const float* bt, const float* bias, float* c, int M, int N, int K, void* scratch,
                        mvnerf_stream_t stream);

/* c (N,K) = g (M,N)^T . a (M,K): the weight gradient of a Dense layer with both operands as they lie (rows = the M samples that are
 * contracted), same kernel family and determinism as mvnerf_gemm_nt.  M % 8 == 0, N % 32 == 0, K % 64 == 0;
 * scratch: mvnerf_gemm_tn_scratch_bytes(M,N,K) bytes. */
size_t mvnerf_gemm_tn_scratch_bytes(int M, int N, int K);
int mvnerf_gemm_tn(const float* g, const float* a, float* c, int M, int N, int K, void* scratch, mvnerf_stream_t stream);

/* A batch of such weight gradients that share M, in one launch (+ one fixed-order reduce): for b < batch
 *     c[b] (N,K) = G[b]^T A[b]  (+ G2[b]^T A2[b]),      colsum[b][n] = sum_m Gs[b][m][n]   (the bias gradient; Gs = G or G2)
 * with G[b] = g + b * g_batch_stride (floats) and row stride ldg - a column block of a wider matrix is used where it lies -, likewise
 * A, G2, A2.  This is what the weight gradients of GraspReadout's per-point layers need (delta_ngf/layers.py:8-42 under the nested tapes
 * of lmvnerf/model_v4.py:290-322): four Dense(128 -> 64) on column blocks of one cotangent, and in the second-order pass the sum of two
 * products per layer.  g2 / a2 may be NULL (one product).  colsum_of: 0 none, 1 G, 2 G2; colsum: batch * N floats.
 * M % 8 == 0, N % 32 == 0, K % 64 == 0; scratch: mvnerf_gemm_tn_batched_scratch_bytes(M,N,K,batch,colsum_of != 0) bytes. */
typedef struct mvnerf_gemm_tn_batch {
    const float* g;  const float* a;  const float* g2;  const float* a2;
    long g_batch_stride, a_batch_stride, g2_batch_stride, a2_batch_stride;
    int ldg, lda, ldg2, lda2;
    int colsum_of;
} mvnerf_gemm_tn_batch;
size_t mvnerf_gemm_tn_batched_scratch_bytes(int M, int N, int K, int batch, int with_colsum);
int mvnerf_gemm_tn_batched(const mvnerf_gemm_tn_batch* q, float* c, float* colsum, int M, int N, int K, int batch, void* scratch,
                           mvnerf_stream_t stream);

/* ---- The trunk as a differentiable field on arbitrary query points. ----
 * Reference consumer: LanguageNeRF._call (lmvnerf/model_v4.py:208-265) evaluates fine_embedding on
 * camera_points / camera_directions derived from grasp poses and keeps outputs[4:] = (view mean, u1, u2, u3)
 * (layers.py:376-377); its train_step (:277-322) takes d prediction / d pose inside a second tape and differentiates a
 * loss on that gradient w.r.t. the read-out, i.e. it needs the trunk's input-gradient (VJP) and the derivative of that
 * VJP w.r.t. its cotangent, which is the forward-mode product (JVP).  The trunk's weights are frozen there.
 * points, dirs: (B,N,3) world space (cam point = E^-1 [p;1], cam dir = (E^-1 [d;1])[:3], Q3) - the forward value is
 * mvnerf_field_eval(rays_o = points, rays_d = dirs, z = 0, S = 1, acts_fused = ...).
 *
 * mvnerf_query_jvp: tangents t_points, t_dirs (B,N,3) -> t_acts (4,B,N,128) = J [t_points; t_dirs]; acts (optional,
 *   may be NULL) receives the primal (4,B,N,128).  workspace: mvnerf_query_workspace_bytes(B,V,N).
 * mvnerf_query_vjp: cotangents g_acts (4,B,N,128) -> d_points, d_dirs (B,N,3) = J^T g_acts.  stash: from
 *   mvnerf_field_eval_stash on the same inputs (R = N, S = 1, z = zeros); bwd_streams: mvnerf_pack_bwd_streams;
 *   scratch: mvnerf_query_vjp_scratch_bytes(B,V,N), 16-byte aligned.  N % 32 == 0 when V > 1. */
size_t mvnerf_query_workspace_bytes(int B, int V, int N);
int mvnerf_query_jvp(const float* points, const float* dirs, const float* t_points, const float* t_dirs,
                     const float* images, const float* features, const float* intrinsics, const float* extrinsics_inv,
                     const float* packed_net, int B, int V, int N, int H, int W, float* acts, float* t_acts, void* workspace,
                     mvnerf_stream_t stream);
size_t mvnerf_query_vjp_scratch_bytes(int B, int V, int N);
int mvnerf_query_vjp(const float* points, const float* dirs, const float* images, const float* features,
                     const float* intrinsics, const float* extrinsics_inv, const float* bwd_streams, const float* stash,
                     const float* g_acts, int B, int V, int N, int H, int W, void* scratch, float* d_points, float* d_dirs,
                     mvnerf_stream_t stream);

/* ---- The same field with its hidden layers on the bf16 matrix pipe (bf16 weights and MFMA inputs, fp32 accumulate: BASELINE.json
 * config 3), for consumers that wait on the trunk's input gradient at inference time (DNGFOptimizer.optimize_pose,
 * lmvnerf/grasp_optimizer.py:158-184, through LanguageNeRF._call, lmvnerf/model_v4.py:208-265).  The frozen trunk's backward needs one
 * thing from the forward, the sign of each pre-activation (ResNetMLPBlock, layers.py:229-231: relu in front of both Dense layers), so the
 * forward keeps 1 bit where mvnerf_field_eval_stash keeps an fp32 value.
 *
 * relu_bits: mvnerf_relu_bits_bytes(B,V,N) bytes, 16-byte aligned.  One bit per pre-activation, [fp32 accumulator > 0], for the 6 per-view
 *   tensors x0,h1,x1,h2,x2,h3 (the mvnerf_stash_bytes slots without x3) and the 6 fused tensors mean,h4,x4,h5,x5,h6 (without x6).
 *   64-bit words [view tile (b V + v) tiles_per_b + k][6][64], then [tile b tiles_per_b + k][6][64]; a tile is 32 consecutive points.
 *   Word `lane` = (j = lane % 32, h = lane / 32) of a (tile, tensor) belongs to point j of the tile; its bit 16 nb + r is feature
 *   32 nb + 8 (r / 4) + 4 h + r % 4: the accumulator register r of output block nb that lane holds in both kernels.
 * mvnerf_pack_bwd_streams_bf16: the twelve hidden kernels transposed, each fp32 weight rounded once to the nearest-even bf16 (the values of
 *   mvnerf_pack_net_bf16), as the A-operand stream of the backward walk: 32 KiB per layer, block 5 (second Dense, first Dense), 4, ... 0.
 * mvnerf_query_stash_bf16: the forward; acts (4,B,N,128) = view mean, u1, u2, u3 as rows, relu_bits as above.  packed16:
 *   mvnerf_pack_net_bf16; workspace: mvnerf_query_workspace_bytes(B,V,N).
 * mvnerf_trunk_vjp_bf16: cotangents g_acts (4,B,N,128) -> g0_tl = dL/d(layer-0 output) in tile layout [view tile][128][32]
 *   (mvnerf_query_vjp_bf16_scratch_bytes(B,V,N) bytes), one launch.  Per block, walking backwards: g_rh = bf16(g) W2^T,
 *   g_hid = g_rh o bits(h), g_x = g + (bf16(g_hid) W1^T) o bits(x), accumulation and residual add in fp32; the cotangents of u3, u2, u1
 *   and the mean enter in fp32 where those tensors are produced (the order of mvnerf_query_vjp); the mean's goes to each view as g / V
 *   (reduce_mean, layers.py:368-370).
 * mvnerf_query_vjp_bf16: that launch followed by the fp32 layer-0 pass of mvnerf_query_vjp (bwd_streams: mvnerf_pack_bwd_streams, of which
 *   only the layer-0 slabs are read) -> d_points, d_dirs (B,N,3).
 * All three: N % 32 == 0 when V > 1, at most 262143 view tiles.  No gradient of the gradient: the second derivative stays fp32
 *   (mvnerf_query_jvp). */
size_t mvnerf_relu_bits_bytes(int B, int V, int N);
size_t mvnerf_bwd_streams_bf16_bytes(void);
int mvnerf_pack_bwd_streams_bf16(const float* net_keras, void* bwd16, mvnerf_stream_t stream);
int mvnerf_query_stash_bf16(const float* points, const float* dirs, const float* images, const float* features, const float* intrinsics,
                            const float* extrinsics_inv, const float* packed_net, const void* packed16, int B, int V, int N, int H, int W,
                            float* acts, void* relu_bits, void* workspace, mvnerf_stream_t stream);
int mvnerf_trunk_vjp_bf16(const void* bwd16, const void* relu_bits, const float* g_acts, int B, int V, int N, float* g0_tl,
                          mvnerf_stream_t stream);
size_t mvnerf_query_vjp_bf16_scratch_bytes(int B, int V, int N);
int mvnerf_query_vjp_bf16(const float* points, const float* dirs, const float* images, const float* features, const float* intrinsics,
                          const float* extrinsics_inv, const float* bwd_streams, const void* bwd16, const void* relu_bits,
                          const float* g_acts, int B, int V, int N, int H, int W, void* scratch, float* d_points, float* d_dirs,
                          mvnerf_stream_t stream);

/* The four fused activations (view mean, u1, u2, u3 - layers.py:376-377, what LanguageNeRF._call keeps as outputs[4:],
 * lmvnerf/model_v4.py:261-262) of a stash written by mvnerf_field_eval_stash with R = N, S = 1, as row-major acts (4, B*N, 128):
 * the stash holds them in the tile layout [tile][feature][32 points]; one transposing pass through LDS.  acts 16-byte aligned. */
int mvnerf_stash_fused_acts(const float* stash, int B, int V, int N, float* acts, mvnerf_stream_t stream);

/* optimize(): clip-by-value (clip > 0) then one Adam step with the bias-corrected rate lr_t.
 * update_mask (optional): n bytes, 0 = leave the element untouched. */
int mvnerf_adam_clip(float* param, const float* grad, float* m, float* v, long n, float lr_t, float beta1, float beta2,
                     float eps, float clip, const unsigned char* update_mask, mvnerf_stream_t stream);

/* ---- the per-point part of GraspReadout (delta_ngf/layers.py:8-42: four Dense(128 -> 64) + elu on the four fused trunk activations,
 * concatenation, Dense(256 -> 64) + elu - what LanguageNeRF._call feeds to the per-pose ResNet blocks, lmvnerf/model_v4.py:261-263) as three
 * fused passes: its value, its vector-Jacobian product and the derivative of that product, which the nested GradientTape of
 * LanguageNeRF.train_step (lmvnerf/model_v4.py:290-322) needs.  fp32, v_mfma_f32_32x32x2_f32, one wavefront per 32 points, row-major (N, F)
 * tensors, 16-byte aligned.  w4: the four Dense kernels (4, 64, 128) [out, in] (torch layout), wc: (64, 256), b4: (4, 64), bc: (64). */
size_t mvnerf_grasp_head_packed_floats(void);
int mvnerf_grasp_head_pack(const float* w4, const float* wc, float* packed, mvnerf_stream_t stream);
/* acts (4, N, 128) -> c (N, 256) = [elu(W_k a_k + b_k)] and y (N, 64) = elu(W_c c + b_c). */
int mvnerf_grasp_head_fwd(const float* acts, const float* packed, const float* b4, const float* bc, long N, float* c, float* y,
                          mvnerf_stream_t stream);
/* g_y (N, 64) = dL/dy -> g_acts (4, N, 128) = dL/d(acts), and the per-point cotangents g_v (N, 64), q (N, 256), g_u (N, 256) from which the
 * weight gradients are skinny GEMMs: dW_c = g_v^T c, db_c = sum g_v, dW_k = g_u[:, 64k:64k+64]^T a_k, db_k = sum g_u[:, 64k:64k+64]. */
int mvnerf_grasp_head_vjp(const float* g_y, const float* c, const float* y, const float* packed, long N, float* g_v, float* q, float* g_u,
                          float* g_acts, mvnerf_stream_t stream);
/* mvnerf_grasp_head_vjp for a frozen read-out (the grasp-pose optimiser): the same products in the same order, only g_acts (4, N, 128) is
 * written - bit-identical to mvnerf_grasp_head_vjp's g_acts, without the 576 floats per point of g_v, q, g_u. */
int mvnerf_grasp_head_vjp_acts(const float* g_y, const float* c, const float* y, const float* packed, long N, float* g_acts,
                               mvnerf_stream_t stream);
/* The derivative of mvnerf_grasp_head_vjp: t_acts (4, N, 128) = dL/d(g_acts) -> out_gy (N, 64) = dL/d(g_y) and r (N, 256), m (N, 64),
 * p (N, 256) with dL/dW_k = g_u_k^T t_k + p_k^T a_k, dL/db_k = sum p_k, dL/dW_c = g_v^T r + m^T c, dL/db_c = sum m. */
int mvnerf_grasp_head_vjp_bwd(const float* t_acts, const float* g_y, const float* c, const float* y, const float* q, const float* packed, long N,
                              float* out_gy, float* r, float* m, float* p, mvnerf_stream_t stream);

/* ---- the per-pose part of GraspReadout (delta_ngf/layers.py:24-28, 39-41; ResNetMLPBlock, mvnerf/layers.py:262-298) with frozen weights:
 * for M = B * P rows x (M, K = 64 n5) = the head's y viewed 'b np n5 d -> (b np) (n5 d)',
 *     h0 = elu(x) W0^T + b0 (K -> 128);  x1 = x Ws^T + elu(h0) W1^T + b1 (-> 64);  h1 = elu(x1) W0'^T + b0';  x2 = x1 + elu(h1) W1'^T + b1';
 *     success = relu(x2) . w_out + b_out.
 * fp32 (v_mfma_f32_32x32x2_f32), one workgroup per 32 rows, no sums across workgroups: the same bits from run to run.  Any M >= 1, n5 >= 1.
 * Weights in torch layout [out, in]: w0 (128, K), b0 (128), w1 (64, 128), b1 (64), ws (64, K) = block_0's shortcut, w0b, w1b (64, 64),
 * b0b, b1b (64) = block_1, w_out (64), b_out (1) or NULL (a read-out without bias).  packed: mvnerf_grasp_tail_packed_floats(n5) floats. */
size_t mvnerf_grasp_tail_packed_floats(int n5);
int mvnerf_grasp_tail_pack(const float* w0, const float* b0, const float* w1, const float* b1, const float* ws, const float* w0b, const float* b0b,
                           const float* w1b, const float* b1b, const float* w_out, const float* b_out, int n5, float* packed,
                           mvnerf_stream_t stream);
/* x (M, 64 n5) -> success (M).  stash (optional): (M, 320) floats = the pre-activations [h0 | x1 | h1 | x2] mvnerf_grasp_tail_vjp reads;
 * NULL = value only.  x, packed, stash 16-byte aligned. */
int mvnerf_grasp_tail_fwd(const float* x, const float* packed, long M, int n5, float* success, float* stash, mvnerf_stream_t stream);
/* g_s (M) = d L / d success (NULL = ones: L = sum of success) -> g_x (M, 64 n5) = (g_h0 W0) . elu'(x) + g_x1 Ws, with elu' taken from x
 * and g_h0, g_x1 from the stashed chain.  x, stash: as given to / written by mvnerf_grasp_tail_fwd. */
int mvnerf_grasp_tail_vjp(const float* x, const float* g_s, const float* stash, const float* packed, long M, int n5, float* g_x,
                          mvnerf_stream_t stream);

/* The same part with TRAINABLE weights: what LanguageNeRF.train_step differentiates (lmvnerf/model_v4.py:277-322: the first backward, and the
 * derivative of the first backward that the nested GradientTape takes).  E = elu, E'(v) = v > 0 ? 1 : e^v, E''(v) = v > 0 ? 0 : e^v,
 * H = [x2 > 0]; x, stash, packed as for mvnerf_grasp_tail_vjp; every (M, .) buffer row-major and 16-byte aligned (g_s, out_gs: 4); rows
 * past M are neither read into results nor written; no sums across workgroups, so the same bits from run to run.  Any M >= 1, n5 >= 1.
 *
 * mvnerf_grasp_tail_vjp_train: g_s (M) or NULL (ones) ->
 *     g_x (M, K)    the same bits mvnerf_grasp_tail_vjp writes for the same inputs,
 *     cot (M, 320)  = [g_h0 (128) | g_x1 (64) | g_h1 (64) | g_x2 (64)], the cotangents of the stashed pre-activations,
 *     act (M, 320)  = [E(h0) | E(x1) | E(h1) | g_s relu(x2)],
 *     ex  (M, K)    = E(x).
 * The weight gradients are skinny TN products of these buffers, formed by the caller (mvnerf_gemm_tn_batched takes the column blocks in place):
 *     dW0 = g_h0^T ex, db0 = sum g_h0;  dW1 = g_x1^T E(h0), db1 = sum g_x1;  dWs = g_x1^T x;  dW0' = g_h1^T E(x1), db0' = sum g_h1;
 *     dW1' = g_x2^T E(h1), db1' = sum g_x2;  dw_out = sum_m g_s relu(x2);  db_out = sum g_s. */
int mvnerf_grasp_tail_vjp_train(const float* x, const float* g_s, const float* stash, const float* packed, long M, int n5, float* g_x, float* cot,
                                float* act, float* ex, mvnerf_stream_t stream);
/* The derivative of mvnerf_grasp_tail_vjp_train: t_x (M, K) = dL/d(g_x) -> the gradient of phi = <t_x, g_x>; cot as written by
 * mvnerf_grasp_tail_vjp_train for the same x, g_s, stash, packed.  Tangents  da0 = E'(x) . t;  dh0 = da0 W0^T;  de0 = E'(h0) . dh0;
 * dx1 = t Ws^T + de0 W1^T;  da1 = E'(x1) . dx1;  dh1 = da1 W0'^T;  de1 = E'(h1) . dh1;  dx2 = dx1 + de1 W1'^T,  and second-order cotangents
 *     pi_h1 = E''(h1) . dh1 . (g_x2 W1');  pi_x1 = E'(x1) . (pi_h1 W0') + E''(x1) . dx1 . (g_h1 W0');
 *     pi_h0 = E'(h0) . (pi_x1 W1) + E''(h0) . dh0 . (g_x1 W1).
 * Outputs:
 *     out_gs (M)      = dphi/dg_s = (H . dx2) . w_out,
 *     out_x  (M, K)   = dphi/dx = E'(x) . (pi_h0 W0) + E''(x) . t . (g_h0 W0) + pi_x1 Ws;  NULL: not formed (one launch instead of two),
 *     cot2   (M, 256) = [pi_h0 (128) | pi_x1 (64) | pi_h1 (64)],
 *     tan    (M, 320) = [de0 (128) | da1 (64) | de1 (64) | g_s H . dx2 (64)],
 *     dex    (M, K)   = da0.
 * Weight gradients of phi, each the sum of two TN products (the g2 / a2 form of mvnerf_gemm_tn_batched):
 *     ddW0 = g_h0^T da0 + pi_h0^T E(x), ddb0 = sum pi_h0;  ddW1 = g_x1^T de0 + pi_x1^T E(h0), ddb1 = sum pi_x1;  ddWs = g_x1^T t + pi_x1^T x;
 *     ddW0' = g_h1^T da1 + pi_h1^T E(x1), ddb0' = sum pi_h1;  ddW1' = g_x2^T de1;  ddw_out = sum_m g_s H . dx2;  ddb1' = ddb_out = 0. */
int mvnerf_grasp_tail_vjp_bwd(const float* x, const float* t_x, const float* g_s, const float* stash, const float* cot, const float* packed, long M,
                              int n5, float* out_gs, float* out_x, float* cot2, float* tan, float* dex, mvnerf_stream_t stream);

/* ---- the grasp-pose optimiser (DNGFOptimizer, lmvnerf/grasp_optimizer.py:28-184; its loop, utils/optimization.py:40-152): the pose side
 * of one optimisation step.  P poses: t (P, 3), rot (P, 4) quaternion (x, y, z, w; rep 0) or (P, 6) 6d ([r1 | r2]; rep 1); offsets (n5, 4, 4)
 * = LanguageNeRF.transforms_to_check (model_v4.py:67-101).  The query tensors hold B scenes of `ld` rows (ld >= P * n5, padding rows are
 * left alone), row p * n5 + o = (pose p, offset o). */

/* compute_matrices (grasp_optimizer.py:113-124: tfg from_quaternion with q as given, or the 6d form normalise-and-cross) followed by
 * LanguageNeRF._query_points (model_v4.py:222-226): points[b, p n5 + o] = R_p t_o + t_p, dirs[b, p n5 + o] = R_p z_o, the same for
 * every scene b (the reference tiles the matrices over B, grasp_optimizer.py:97-98).  points, dirs: (B, ld, 3). */
int mvnerf_pose_query_points(const float* t, const float* rot, int rep, const float* offsets, int P, int n5, int B, long ld, float* points,
                             float* dirs, mvnerf_stream_t stream);
/* The vector-Jacobian product of mvnerf_pose_query_points: d_points, d_dirs (B, ld, 3) -> d_t (P, 3), d_rot (P, 4|6), both multiplied by
 * `scale` (-1: the gradient of loss = -success, grasp_optimizer.py:177).  Fixed-order sums (bit-identical from run to run). */
int mvnerf_pose_query_vjp(const float* rot, int rep, const float* offsets, const float* d_points, const float* d_dirs, int P, int n5, int B,
                          long ld, float scale, float* d_t, float* d_rot, mvnerf_stream_t stream);

/* The forward-mode product of mvnerf_pose_query_points along (c_t (P, 3), c_rot (P, 4|6)): t_points[b, p n5 + o] = dR_p t_o + c_t_p,
 * t_dirs[b, p n5 + o] = dR_p z_o, (B, ld, 3) each, rows past P * n5 of a scene left alone.  dR is the derivative of the tfg quaternion form
 * with q as given (not normalised), or of the 6d form through x / |x| of both halves and their cross product.  It is also the derivative
 * of mvnerf_pose_query_vjp w.r.t. its cotangents, which is what LanguageNeRF.train_step's nested tape takes of the pose map
 * (lmvnerf/model_v4.py:290-322; compute_matrices :192-206, the query points :222-226). */
int mvnerf_pose_query_jvp(const float* rot, int rep, const float* offsets, const float* c_t, const float* c_rot, int P, int n5, int B, long ld,
                          float* t_points, float* t_dirs, mvnerf_stream_t stream);

/* optimize(opt, var, g, 1.0) for each trained variable (grasp_optimizer.py:179-182; nerf_utils.py:8-12: clip-by-value, then
 * tf.keras.optimizers.Adam with ExponentialDecay(lr0, decay_steps=1, decay, staircase=False), optimization.py:47-61), then post_process
 * (grasp_optimizer.py:126-139) of every pose.  Step k of variable v uses lr = lr0[v] decay[v]^(k-1), alpha = lr sqrt(1 - beta2^k) /
 * (1 - beta1^k); m += (g - m)(1 - beta1); v += (g^2 - v)(1 - beta2); x -= alpha m / (sqrt(v) + eps).
 * train_flags (2) int32: variable 0 = t, 1 = rot is stepped when non-zero.  counters (2, P) int32: the step count k of each variable, per
 * pose, advanced on the device by the thread that owns the pose (the two Keras optimisers' `iterations`).  Nothing per step comes from the
 * host: a captured step serves both phases, the caller switches them by writing train_flags on the stream. */
typedef struct mvnerf_pose_adam_config {
    float lr0[2], decay[2];            /* [0] translations, [1] rotations */
    float beta1, beta2, eps, clip;     /* clip <= 0: no clip-by-value */
    int clip_translation;              /* clip t to [lo, hi] per axis (workspace_bounds) */
    float lo[3], hi[3];
} mvnerf_pose_adam_config;
/* cfg is [host]; g_t, m_t, v_t, t: (P, 3); g_rot, m_r, v_r, rot: (P, 4|6).  In place on t, rot, m_*, v_*, counters. */
int mvnerf_pose_adam_step(const mvnerf_pose_adam_config* cfg, int rep, int P, const int* train_flags, int* counters, const float* g_t,
                          const float* g_rot, float* m_t, float* v_t, float* m_r, float* v_r, float* t, float* rot, mvnerf_stream_t stream);

/* ---- one grasp-pose optimisation step behind one call (DNGFOptimizer.optimize_pose, lmvnerf/grasp_optimizer.py:158-184, through
 * LanguageNeRF._call, lmvnerf/model_v4.py:208-265): poses -> query points -> frozen trunk with stash -> GraspReadout (head, per-pose tail) ->
 * success, and back: tail VJP -> head VJP -> trunk VJP -> pose VJP -> clip, Keras Adam, post_process.  Nothing is allocated, nothing
 * synchronises with the host, every launch goes to `stream`: a step can be captured in a HIP graph (the phase switches through the
 * device-resident train_flags).  For V > 1 every scene's P * n5 rows are padded to whole 32-point tiles inside the workspace (the last point
 * repeated, its cotangents zero). */
typedef struct mvnerf_grasp_call {
    /* the scene: device pointers, layouts as in mvnerf_query_vjp */
    const float* images;          /* (B,V,H,W,3) */
    const float* features;        /* (B,V,H,W,256) */
    const float* intrinsics;      /* (B,V,4,4) */
    const float* extrinsics_inv;  /* (B,V,4,4) */
    int B, V, H, W;
    /* the frozen trunk */
    const float* packed_net;      /* mvnerf_pack_net */
    const void* split;            /* mvnerf_pack_net_split */
    const float* bwd_streams;     /* mvnerf_pack_bwd_streams */
    /* the frozen read-out */
    const float* head_packed;     /* mvnerf_grasp_head_pack */
    const float* head_b4;         /* (4, 64) */
    const float* head_bc;         /* (64) */
    const float* tail_packed;     /* mvnerf_grasp_tail_pack for the same n5 */
    const float* offsets;         /* (n5, 4, 4) transforms_to_check */
    int rep, P, n5;               /* rep: 0 quaternion (x, y, z, w), 1 6d */
    /* the pose state (updated in place by mvnerf_grasp_opt_step) and the outputs */
    float* t;                     /* (P, 3) */
    float* rot;                   /* (P, 4 | 6) */
    float* success;               /* (B, P): the poses' predicted success per scene, before the step */
    float* g_t;                   /* (P, 3)     d(-sum success) / d t     (not needed by mvnerf_grasp_success) */
    float* g_rot;                 /* (P, 4 | 6) d(-sum success) / d rot   (likewise) */
    void* workspace;              /* 256-byte aligned, >= mvnerf_grasp_workspace_bytes(B, V, P, n5) */
    size_t workspace_bytes;
} mvnerf_grasp_call;

/* Bytes of workspace: points, dirs, zero depths and the field kernel's output and scratch, the trunk stash, the fused activations, the head's
 * c and y, the tail stash, g_x, g_acts, the trunk VJP's scratch and d_points / d_dirs.  0 for non-positive sizes. */
size_t mvnerf_grasp_workspace_bytes(int B, int V, int P, int n5);
/* Stages 1-4, value only: success (B, P)  (DNGFOptimizer.compute_current_grasp_success before its sum over scenes). */
int mvnerf_grasp_success(const mvnerf_grasp_call* call, mvnerf_stream_t stream);
/* Stages 1-7: success, and g_t, g_rot = d(-sum success) / d(t, rot) (grasp_optimizer.py:171-178). */
int mvnerf_grasp_success_and_gradients(const mvnerf_grasp_call* call, mvnerf_stream_t stream);
/* Stages 1-8: the above followed by mvnerf_pose_adam_step on t, rot (arguments as there; cfg is [host]). */
int mvnerf_grasp_opt_step(const mvnerf_grasp_call* call, const mvnerf_pose_adam_config* cfg, const int* train_flags, int* counters, float* m_t,
                          float* v_t, float* m_r, float* v_r, mvnerf_stream_t stream);

/* The same three calls with the trunk on the bf16 matrix pipe (DNGFOptimizer.optimize_pose, lmvnerf/grasp_optimizer.py:158-184, under
 * BASELINE.json config 3): stage 2 is mvnerf_query_stash_bf16, stage 6 mvnerf_query_vjp_bf16, everything else as above.  The call is the
 * same struct (`split` is not read and may be NULL); packed16: mvnerf_pack_net_bf16, bwd16: mvnerf_pack_bwd_streams_bf16, both 16-byte
 * aligned.  workspace: mvnerf_grasp_workspace_bytes_bf16 (relu bits in place of the stash). */
size_t mvnerf_grasp_workspace_bytes_bf16(int B, int V, int P, int n5);
int mvnerf_grasp_success_bf16(const mvnerf_grasp_call* call, const void* packed16, const void* bwd16, mvnerf_stream_t stream);
int mvnerf_grasp_success_and_gradients_bf16(const mvnerf_grasp_call* call, const void* packed16, const void* bwd16, mvnerf_stream_t stream);
int mvnerf_grasp_opt_step_bf16(const mvnerf_grasp_call* call, const void* packed16, const void* bwd16, const mvnerf_pose_adam_config* cfg,
                               const int* train_flags, int* counters, float* m_t, float* v_t, float* m_r, float* v_r, mvnerf_stream_t stream);

/* ---- the losses of LanguageNeRF.train_step (lmvnerf/model_v4.py:277-318) with their cotangents.  One workgroup each, fixed-order sums, no
 * atomics: the same bits from run to run. ---- */
#define MVNERF_LOSS_KL_DIVERGENCE 0   /* softmax over the last axis, then tf.keras.losses.KLDivergence(reduction=NONE): one loss per batch element */
#define MVNERF_LOSS_CROSS_ENTROPY 1   /* tf.keras.losses.CategoricalCrossentropy(from_logits=True): mean over the batch */
/* The landscape loss (model_v4.py:280-285 with the loss train_language.py:40-63 selects) of the predicted success y (B, np) against label
 * (B, np): loss[0] = its mean over the batch, g_y (B, np) = weight * d(total)/dy where total = the sum over the batch (kl_divergence: both
 * inputs clipped to [1e-7, 1], no derivative outside) or the mean (cross_entropy). */
int mvnerf_landscape_loss(const float* y, const float* label, int B, int np, int kind, float weight, float* g_y, float* loss,
                          mvnerf_stream_t stream);
/* tf.keras.losses.CosineSimilarity(axis=-1) as model_v4.py:300-314 uses it on d prediction / d pose: x, label (rows, dim), dim = 3, 4, or
 * 6 = the two 3-halves taken separately and added; loss[0] = -mean_rows sum_halves u(label) . u(x), u(x) = x rsqrt(max(sum x^2, 1e-12));
 * g_x (rows, dim) = scale * d loss / d x. */
int mvnerf_cosine_loss(const float* x, const float* label, long rows, int dim, float scale, float* g_x, float* loss, mvnerf_stream_t stream);

/* ---- the LanguageNeRF training step up to the optimiser behind one call (LanguageNeRF.train_step, lmvnerf/model_v4.py:277-318 through _call
 * :208-265): the landscape loss on one pose set, the cosine losses on d prediction / d pose of a second set (the nested GradientTape,
 * :290-314), and the gradient of their sum w.r.t. the GraspReadout variables (:316-318; delta_ngf/layers.py:8-42).  The trunk is frozen.
 * Nothing is allocated, nothing synchronises with the host, every launch goes to `stream`: a step can be captured in a HIP graph.  Any
 * B, V, np, n5 >= 1: the weight-gradient products pad their row count to a multiple of 8 inside the workspace, and for V > 1 every scene's
 * np * n5 rows are padded to whole 32-point tiles (the last point repeated, its cotangents zero).
 * grads: mvnerf_language_grad_floats(n5) floats, the variables in torch [out, in] orientation, K = 64 n5, in this order:
 *     head   w4 (4, 64, 128), b4 (4, 64), wc (64, 256), bc (64)                             [activation_downscale 0..3, combined_activation_downscale]
 *     tail   w0 (128, K), b0 (128), w1 (64, 128), b1 (64), ws (64, K)                       [block_0: layer_0, layer_1, shortcut]
 *            w0b (64, 64), w1b (64, 64), b0b (64), b1b (64)                                  [block_1: both weights, then both biases]
 *            w_out (64), b_out (1)                                                            [output_layer]
 * scalars (4): landscape_loss (mean over the batch), grad_loss_t, grad_loss_r, pred (mean prediction) - the dict train_step returns (:318).
 * With MVNERF_LOSS_KL_DIVERGENCE the total is one loss per batch element, summed (:316): the two scalar cosine losses enter B times. */
typedef struct mvnerf_language_call {
    /* the scene: device pointers, layouts as in mvnerf_query_vjp */
    const float* images;          /* (B,V,H,W,3) */
    const float* features;        /* (B,V,H,W,256) */
    const float* intrinsics;      /* (B,V,4,4) */
    const float* extrinsics_inv;  /* (B,V,4,4) */
    int B, V, H, W;
    /* the frozen trunk */
    const float* packed_net;      /* mvnerf_pack_net */
    const void* split;            /* mvnerf_pack_net_split */
    const float* bwd_streams;     /* mvnerf_pack_bwd_streams */
    /* the read-out being trained, plain weights (packed by the step: they change every step) */
    const float* head_w4;         /* (4, 64, 128) */
    const float* head_b4;         /* (4, 64) */
    const float* head_wc;         /* (64, 256) */
    const float* head_bc;         /* (64) */
    const float* tail_w[11];      /* w0, b0, w1, b1, ws, w0b, b0b, w1b, b1b, w_out, b_out: the order of mvnerf_grasp_tail_pack */
    const float* offsets;         /* (n5, 4, 4) transforms_to_check */
    int rep, np, n5;              /* rep: 0 quaternion (x, y, z, w), 1 6d; np poses per scene */
    /* the two pose sets (model_v4.py:279, :287) and the labels */
    const float* t_landscape;     /* (B, np, 3) */
    const float* rot_landscape;   /* (B, np, 4 | 6) */
    const float* t_grad;          /* (B, np, 3) */
    const float* rot_grad;        /* (B, np, 4 | 6) */
    const float* label_landscape; /* (B, np) */
    const float* label_grad_t;    /* (B, np, 3) */
    const float* label_grad_r;    /* (B, np, 4 | 6) */
    int loss_kind;                /* MVNERF_LOSS_* */
    float w_land, w_t, w_r;       /* weights of the three losses' cotangents (the reference: 1, 1, 1) */
    /* outputs */
    float* grads;                 /* mvnerf_language_grad_floats(n5), 16-byte aligned */
    float* prediction;            /* (B, np): the read-out on the gradient poses */
    float* scalars;               /* (4) */
    void* workspace;              /* 256-byte aligned, >= mvnerf_language_workspace_bytes(B, V, H, W, np, n5) */
    size_t workspace_bytes;
} mvnerf_language_call;
size_t mvnerf_language_grad_floats(int n5);
/* Bytes of workspace (every intermediate of both passes, the packed read-out, the three gradient contributions).  0 for non-positive sizes. */
size_t mvnerf_language_workspace_bytes(int B, int V, int H, int W, int np, int n5);
int mvnerf_language_loss_and_grads(const mvnerf_language_call* call, mvnerf_stream_t stream);

/* ---- the optimiser of that step (src/train_language.py:65-67: tf.keras.optimizers.Adam, behind optimize() = clip-by-value then Adam,
 * nerf_utils.py:8-12) and the whole step behind one call.  The update is mvnerf_adam_clip's, operation for operation:
 *     g = clip(g);  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;  p = p - lr_t m / (sqrt(v) + eps)
 * with lr_t = (float)(lr sqrt(1 - beta2^t) / (1 - beta1^t)) formed ON THE DEVICE in double from t = *step + 1 (beta^t by square-and-
 * multiply), so that a captured graph needs no host-side rate.  The variables are the 21 tensors the model owns, updated in place where
 * they are; m, v have the flat layout of `grads` above.  Nothing is allocated, nothing synchronises with the host, no atomics. */
typedef struct mvnerf_language_adam {
    float* head_w[4];             /* activation_downscale 0..3 weights (64, 128): the variables themselves */
    float* head_b[4];             /* their biases (64) */
    float* head_wc;               /* combined_activation_downscale (64, 256) = mvnerf_language_call.head_wc */
    float* head_bc;               /* (64) */
    float* tail_w[11];            /* the pointers and the order of mvnerf_language_call.tail_w */
    float* head_w4;               /* (4, 64, 128) the stacked image mvnerf_language_call.head_w4 reads: written from head_w[] */
    float* head_b4;               /* (4, 64) likewise from head_b[] */
    float* m;                     /* mvnerf_language_grad_floats(n5) first moments, the layout of `grads` */
    float* v;                     /* second moments */
    long long* step;              /* one device word, 8-byte aligned: the number of completed updates; read and advanced on the device */
    float lr, beta1, beta2, eps;  /* Keras: lr, 0.9, 0.999, 1e-7; lr is NOT bias-corrected */
    float clip;                   /* clip-by-value bound of optimize(), <= 0: none */
} mvnerf_language_adam;
/* One update from call->grads (only grads and n5 of `call` are read): a launch over the flat index space that clips, updates m, v and the
 * variable an index belongs to and mirrors an updated head_w[] / head_b[] element into head_w4 / head_b4, then a one-thread launch that
 * makes *step one larger - stream-ordered behind every read of it. */
int mvnerf_language_apply_gradients(const mvnerf_language_call* call, const mvnerf_language_adam* adam, mvnerf_stream_t stream);
/* LanguageNeRF.train_step on one device: head_w[] / head_b[] gathered into head_w4 / head_b4 (so a caller that rewrote the variables in
 * place needs no invalidation call), mvnerf_language_loss_and_grads, mvnerf_language_apply_gradients.  The 15 weight pointers of `adam`
 * must be those of `call`. */
int mvnerf_language_train_step(const mvnerf_language_call* call, const mvnerf_language_adam* adam, mvnerf_stream_t stream);

/* ---- the whole training step behind one call (MVVNeRFRenderer.train_step, model_v0.py:186-197: GradientTape over call(),
 * loss = MSE(y, rgb) + MSE(y, fine_rgb) :193, gradients :194, optimize() :195 = nerf_utils.py:8-12) ----
 * The matching `_bwd` of mvnerf_render_fwd: a host in any language takes a training step with these entry points and
 * a caller-provided workspace; nothing is allocated, nothing synchronises with the host. */
typedef struct mvnerf_train_call {
    /* inputs of _call (model_v0.py:113-119): device pointers, layouts as in mvnerf_render_fwd */
    const float* rays_o;          /* (B,R,3) */
    const float* rays_d;          /* (B,R,3) */
    const float* images;          /* (B,V,H,W,3) in [0,1] */
    const float* features;        /* (B,V,H,W,256) combined_features */
    const float* intrinsics;      /* (B,V,4,4) */
    const float* extrinsics_inv;  /* (B,V,4,4) */
    const float* u_coarse;        /* (B,R,64) the uniforms of sample_along_ray (nerf_utils.py:57) */
    const float* u_fine;          /* (B,R,64) the uniforms of sample_pdf (nerf_utils.py:151) */
    const float* labels;          /* (B,R,3) target colours */
    int B, V, R, S, H, W;         /* S = 64 */
    double near_, far_;
    int q7_mode;                  /* MVNERF_Q7_ZERO | MVNERF_Q7_CLAMP */
    int stop_fine_z;              /* 1: cut the gradient through the importance samples (the reference leaves it open) */
    int use_texel_tables;         /* 1: forward (and the position / feature-map gradients) through per-texel layer-0 tables built inside the
                                   * workspace (mvnerf_project_texels2); pays when R*S >= 2*H*W */
    /* the two MLPs: Keras-order variables (247300 floats each) and the images the kernels read, all caller-owned */
    const float* net_coarse;      /* updated in place by mvnerf_apply_gradients / mvnerf_train_step */
    const float* net_fine;
    const float* packed_coarse;   /* mvnerf_pack_net */
    const float* packed_fine;
    const void* split_coarse;     /* mvnerf_pack_net_split, or both NULL: forward on the fp32 MFMA */
    const void* split_fine;
    const float* bwd_streams_coarse;   /* mvnerf_pack_bwd_streams */
    const float* bwd_streams_fine;
    /* outputs */
    float* loss;                  /* 1 float: overwritten */
    float* grad;                  /* 2 x 247300 floats [coarse | fine], Keras order: overwritten */
    float* rgb;                   /* (B,R,3) */
    float* depth;                 /* (B,R) */
    float* fine_rgb;              /* (B,R,3) */
    float* fine_depth;            /* (B,R) */
    float* d_features;            /* optional (B,V,H,W,256): overwritten with dL/d(combined_features) - what flows back to the reference's
                                   * trainable encoders (train_nerf.py:27-32); NULL = not wanted */
    void* workspace;              /* 256-byte aligned, >= mvnerf_train_workspace_bytes(...) */
    size_t workspace_bytes;
    void* fine_grad_event;        /* optional hipEvent_t (NULL = none): recorded on the stream as soon as the FINE net's half of `grad` is
                                   * final, i.e. before the coarse net's backward is launched - a data-parallel host starts that half's
                                   * all-reduce on a second stream behind this event and overlaps it with the coarse backward */
} mvnerf_train_call;

typedef struct mvnerf_adam_state {
    float* m;                     /* 2 x 247300 first moments  [coarse | fine] */
    float* v;                     /* 2 x 247300 second moments */
    float lr_t;                   /* bias-corrected rate lr * sqrt(1 - beta2^t) / (1 - beta1^t) (tf.keras Adam) */
    float beta1, beta2, eps;      /* Keras defaults 0.9, 0.999, 1e-7 */
    float clip;                   /* clip-by-value bound of optimize() (nerf_utils.py:9), <= 0: none */
    const unsigned char* update_mask;   /* optional 2 x 247300 bytes, 0 = variable not in the optimizer's list */
    int repack;                   /* 1: rebuild packed_* / split_* / bwd_streams_* of the call from the updated variables */
} mvnerf_adam_state;

size_t mvnerf_train_workspace_bytes(int B, int V, int R, int S, int H, int W, int use_texel_tables, int want_d_features);
/* Forward with stash + loss + full backward: fills loss, grad, the four rendered outputs (and d_features).  model_v0.py:190-194. */
int mvnerf_loss_and_grads(const mvnerf_train_call* call, mvnerf_stream_t stream);
/* optimize() on `grad` (a data-parallel host all-reduces it first): clip-by-value, Adam, optional re-pack.  nerf_utils.py:8-12. */
int mvnerf_apply_gradients(const mvnerf_train_call* call, const mvnerf_adam_state* adam, mvnerf_stream_t stream);
/* mvnerf_loss_and_grads followed by mvnerf_apply_gradients: MVVNeRFRenderer.train_step on one device. */
int mvnerf_train_step(const mvnerf_train_call* call, const mvnerf_adam_state* adam, mvnerf_stream_t stream);

/* Bytes of scratch mvnerf_render_fwd needs for (B,V,R,S). */
size_t mvnerf_render_workspace_bytes(int B, int V, int R, int S);

/* MVVNeRFRenderer._call (model_v0.py:113-184): stratified depths -> coarse field -> composite ->
 * resample -> fine field -> composite, all on `stream`, no host synchronisation.
 * u_coarse, u_fine (B,R,S) are the uniforms the reference draws inside the graph
 * (nerf_utils.py:57,151), here explicit.  S must be 64.
 * Outputs: rgb, fine_rgb (B,R,3); depth, fine_depth (B,R)  (the reference's 4-tuple, :184).
 * workspace: 16-byte aligned, mvnerf_render_workspace_bytes(B,V,R,S) bytes.
 * texel_tables (optional, may be NULL = gather raw features): 2 x mvnerf_texel_table_bytes(B,V,H,W) bytes, coarse
 * net's table then fine net's.  tables_ready == 0: both are (re)built by this call; != 0: used as they are (same
 * feature maps and nets as the call that built them, e.g. the next ray chunk of the same frame). */
int mvnerf_render_fwd(const float* rays_o, const float* rays_d, const float* images, const float* features,
                      const float* intrinsics, const float* extrinsics_inv, const float* packed_coarse,
                      const float* packed_fine, const float* u_coarse, const float* u_fine, int B, int V,
                      int R, int S, int H, int W, double near_, double far_, int q7_mode, float* rgb,
                      float* depth, float* fine_rgb, float* fine_depth, void* workspace, float* texel_tables,
                      int tables_ready, mvnerf_stream_t stream);

/* mvnerf_render_fwd with both field passes on the split-bf16 kernel (mvnerf_field_eval_split): split_coarse / split_fine =
 * mvnerf_pack_net_split of the two nets; packed_coarse / packed_fine still supply biases, the per-ray layer-0 seed and the
 * texel tables.  Same outputs, same 1e-4 bar. */
int mvnerf_render_fwd_split(const float* rays_o, const float* rays_d, const float* images, const float* features,
                            const float* intrinsics, const float* extrinsics_inv, const float* packed_coarse,
                            const float* packed_fine, const void* split_coarse, const void* split_fine, const float* u_coarse,
                            const float* u_fine, int B, int V, int R, int S, int H, int W, double near_, double far_, int q7_mode,
                            float* rgb, float* depth, float* fine_rgb, float* fine_depth, void* workspace, float* texel_tables,
                            int tables_ready, mvnerf_stream_t stream);
/* ... with `which` and `range_status` as in mvnerf_field_eval_split_ex; range_status here is TWO floats: [0] the coarse pass, [1] the fine pass. */
int mvnerf_render_fwd_split_ex(const float* rays_o, const float* rays_d, const float* images, const float* features,
                               const float* intrinsics, const float* extrinsics_inv, const float* packed_coarse,
                               const float* packed_fine, const void* split_coarse, const void* split_fine, const float* u_coarse,
                               const float* u_fine, int B, int V, int R, int S, int H, int W, double near_, double far_, int q7_mode,
                               float* rgb, float* depth, float* fine_rgb, float* fine_depth, void* workspace, float* texel_tables,
                               int tables_ready, int which, float* range_status, mvnerf_stream_t stream);

/* The tail of both feature producers as one launch (layers.py:459-477 ConvFusion + :617-618,658-659 UpSampling2D(bilinear);
 * legacy_layers.py:154-191 CombineCLIPVisualV0):  out = bilinear_x2( act([a | b]) . weight ).
 * a (N,h,w,Ca), b (N,h,w,Cb): fp32, NHWC contiguous, concatenated in that order; weight (Ca+Cb, 256) row-major, the Keras
 * (1,1,Cin,256) kernel as stored.  act: 0 identity, 1 relu, 2 elu (alpha 1), applied to the concatenated input before the product.
 * out (N,2h,2w,256) NHWC: fp32, or bf16 (round to nearest even, the last operation) when out_bf16 != 0.  The product is exact-fp32 MFMA
 * with fp32 accumulation in a fixed order; the up-sampling uses half-pixel centres with clamped indices (weights 3/4, 1/4).  The
 * low-resolution product never reaches global memory: no workspace, no atomics, bit-identical from run to run.
 * Ca, Cb: multiples of 16, each >= 16, Ca + Cb <= 512 (else MVNERF_E_SHAPE; so is act outside 0..2).  All four pointers 16-byte aligned. */
int mvnerf_fuse_upsample2x(const float* a, const float* b, const float* weight, int N, int h, int w, int Ca, int Cb, int act,
                           void* out, int out_bf16, mvnerf_stream_t stream);

/* The backward of mvnerf_fuse_upsample2x as one launch.  g = dL/dout (N,2h,2w,256) fp32 NHWC; a, b, weight as in the forward:
 *   g_low[n,y,x,c] = sum_{Y,X'} cy(Y,y) cx(X',x) g[n,Y,X',c]       the adjoint of the x2 bilinear up-sampling (half-pixel centres, clamped
 *                                                                 taps; the two taps that clamp onto one border sample add to 1)
 *   dX[n,y,x,k]    = act'(X[n,y,x,k]) * sum_c g_low[n,y,x,c] weight[k,c],   X = [a | b];   da = dX[..., :Ca],  db = dX[..., Ca:]
 * da (N,h,w,Ca), db (N,h,w,Cb), g_low (N,h,w,256): each may be NULL (not wanted; only the requested halves are computed); all three NULL
 * is MVNERF_E_ARG.  g_low is the copy of the adjoint a weight gradient needs: dW = act(X)^T . g_low.  a (b) may be NULL where act == 0 or
 * da (db) is NULL: the identity does not read them.  A low pixel gathers its <= 4 x 4 outputs in a fixed order (rows first, then columns,
 * ascending; csrc/mvnerf_feature_tail.h), one rounding per written operation; the product is exact-fp32 MFMA, summed over the 256 channels
 * in a fixed order.  No atomics, no workspace, no host read: bit-identical from run to run, and capturable.  A NaN in g reaches only the
 * <= 2 x 2 low pixels it feeds.  Shape rules of the forward (Ca, Cb multiples of 16, each >= 16, Ca + Cb <= 512, act 0..2: else
 * MVNERF_E_SHAPE); every non-NULL pointer 16-byte aligned. */
int mvnerf_fuse_upsample2x_bwd(const float* g, const float* a, const float* b, const float* weight, int N, int h, int w, int Ca, int Cb,
                               int act, float* da, float* db, float* g_low, mvnerf_stream_t stream);

/* ---- 3x3 convolutions of the language fusion (layers.py:414-456 DoubleConv / Up, :593-660 CombineCLIPVisualV4) as one launch each:
 *   out[n,i,j,co] = mul[n,co] * act( sum_{dy,dx in 0..2} sum_c X[n, i+dy-1, j+dx-1, c] * W[dy,dx,c,co] ),   X = [a | b] along c
 * Conv2D(3, padding='same', use_bias=False), stride 1; taps outside the image are 0; images of a batch do not see each other.
 * Products at fp32 grade on the fp16 matrix pipe: both operands as two fp16 pieces under a per-tensor power-of-two scale, three
 * v_mfma_f32_16x16x32_f16 per product block, fp32 accumulation in a fixed order.  No atomics on out, no workspace:
 * bit-identical from run to run. */

/* Bytes of the packed weight stream of a (3,3,cin,cout) kernel; 0 when the channel counts are not accepted (cin % 32, cout % 64). */
size_t mvnerf_conv3x3_packed_bytes(int cin, int cout);

/* w_hwio (3,3,cin,cout) fp32, the Keras kernel as stored -> `packed` (16-byte aligned, mvnerf_conv3x3_packed_bytes): a 256-byte header
 * (max |w| found on the device, the scale exponent derived from it) and the fp16 pieces in the order the kernel consumes them.
 * Stream-ordered, no host read.  Call once per weight update. */
int mvnerf_conv3x3_pack(const float* w_hwio, int cin, int cout, void* packed, mvnerf_stream_t stream);

/* *amax = max |x| over n floats (the word is overwritten).  A NaN in x gives a NaN; for maps that another library produced. */
int mvnerf_absmax_f32(const float* x, long n, float* amax, mvnerf_stream_t stream);

/* a (N,h,w,Ca), b (N,h,w,Cb) or NULL with Cb = 0: fp32 NHWC, concatenated in that order without a copy.  amax_a, amax_b: one device
 * float each, an UPPER BOUND of |a|, |b| (mvnerf_absmax_f32, or the amax_out of the launch that wrote the map): the kernel derives the
 * operand scales from them.  A bound of 0 means an all-zero source; a non-finite bound fills out with NaN.  packed: mvnerf_conv3x3_pack
 * of the (3,3,Ca+Cb,Cout) kernel.  act: 0 identity, 1 relu, 2 elu (alpha 1), applied to the sum; mul (N,Cout) or NULL multiplies after
 * the activation.  out (N,h,w,Cout) fp32 NHWC.  amax_out (optional): one device word the CALLER ZEROES; on return max |out| (a NaN
 * written anywhere makes it a NaN).
 * Ca, Cb multiples of 32 (Ca >= 32), Cout a multiple of 64, act in 0..2: else MVNERF_E_SHAPE, before any launch.  a, b, packed, mul, out
 * 16-byte aligned. */
int mvnerf_conv3x3_nhwc(const float* a, int Ca, const float* amax_a, const float* b, int Cb, const float* amax_b, const void* packed,
                        int N, int h, int w, int Cout, int act, const float* mul, float* out, float* amax_out, mvnerf_stream_t stream);

/* ---- the 3x3 convolutions of VisualFeatures (layers.py:7-34 Block, :37-57 ConvolutionalEncoder, :150-229 VisionTransformerEncoder):
 * Conv2D(3, padding='same') WITH a bias, a relu in front of a convolution (output_conv, layers.py:206-212), and
 * BatchNormalization(training=True) behind it (Block, layers.py:22-27).  Inference only. */

/* mvnerf_conv3x3_nhwc with three more arguments (everything else as above; with bias = NULL, act_in = 0, stats = NULL it IS that call):
 *   bias    (Cout) fp32 or NULL: out = mul * act(sum + bias[co]) - added to the un-scaled sum, before act.  amax_out covers what is
 *           written.  16-byte aligned.
 *   act_in  0 identity, 1 relu, 2 elu: applied to every element of a and b as it is read, before the fp16 cut.  |relu(x)| <= |x| and
 *           |elu(x)| <= |x|, so amax_a / amax_b computed on the un-activated sources stay valid bounds.  Taps outside the image are
 *           zero AFTER the activation (Keras pads the activated map).
 *   stats   NULL, or mvnerf_conv3x3_stats_bytes bytes (16-byte aligned): for every workgroup - channel tile ct of 64, image n, tile row
 *           ty, tile column tx of 16 x 16 pixels, in that order - 64 means and then 64 M2 (sums of squared deviations from that mean) of
 *           the values written to the tile's real pixels, per channel.  The mean is reduced first, then the deviations about it; no raw
 *           sum of squares is formed.  Pixel counts follow from (h, w) and are not stored.  Every workgroup owns its slots (plain stores,
 *           no atomics): two runs give the same bits.  A non-finite amax fills them with NaN. */
size_t mvnerf_conv3x3_stats_bytes(int N, int h, int w, int Cout);
int mvnerf_conv3x3_nhwc_ex(const float* a, int Ca, const float* amax_a, const float* b, int Cb, const float* amax_b, const void* packed,
                           int N, int h, int w, int Cout, int act, const float* mul, float* out, float* amax_out, const float* bias,
                           int act_in, float* stats, mvnerf_stream_t stream);

/* ---- backward of the biased 3x3 convolution (csrc/conv3x3_bwd.hip) -------------------------------------------------------------------
 * For y = conv3x3_same(act_in(x), W) + bias and g = dL/dy.  The data gradient needs no entry point of its own: it is
 * mvnerf_conv3x3_nhwc of g with the pack of W'[dy,dx,co,ci] = W[2-dy,2-dx,ci,co] (Cout of the forward a multiple of 32, Cin of 64). */

/* Pixels per slab of the weight gradient's reduction (whole 16 x 16 tiles, in the order [image][tile row][tile column]). */
int mvnerf_conv3x3_wgrad_slab_pixels(void);

/* Bytes of the workspace of mvnerf_conv3x3_wgrad_nhwc: one fp32 partial of dw and dbias per slab; 0 when the shape is not accepted. */
size_t mvnerf_conv3x3_wgrad_workspace_bytes(int N, int h, int w, int Cin, int Cout);

/* dw_hwio (3,3,Cin,Cout) fp32, the Keras layout: dw[dy,dx,ci,co] = sum_{n,i,j} act_in(x)[n,i+dy-1,j+dx-1,ci] * g[n,i,j,co], taps outside
 * the image zero after the activation, images apart; dbias (Cout) or NULL: sum_{n,i,j} g[n,i,j,co].
 * x (N,h,w,Cin), g (N,h,w,Cout): fp32 NHWC.  amax_x, amax_g: one device float each, an UPPER BOUND of |x|, |g| (as for the forward: a
 * bound of |x| bounds |act_in(x)|).  A bound of 0 gives zeros (amax_x = 0 leaves dbias the plain sum), a non-finite bound NaN in dw and
 * dbias.  act_in: 0 identity, 1 relu, 2 elu, applied to x as it is read.
 * fp32 grade on the fp16 matrix pipe: g cut like a weight, act_in(x) like an activation, three products.  The pixels are summed in
 * slabs (fp32 inside a slab, a fixed order), the slabs in a second launch in order in double, then one rounding; dbias likewise from
 * one more small launch.  No atomics, nothing of `workspace` is read that this call did not write: two runs give the same bits.
 * Stream-ordered, no host read.  Cin a multiple of 32, Cout a multiple of 64, act_in in 0..2: else MVNERF_E_SHAPE, before any launch.
 * x, g, dw_hwio, dbias, workspace 16-byte aligned. */
int mvnerf_conv3x3_wgrad_nhwc(const float* x, const float* amax_x, int act_in, const float* g, const float* amax_g, int N, int h, int w,
                              int Cin, int Cout, float* dw_hwio, float* dbias, void* workspace, mvnerf_stream_t stream);

/* ---- backward through a FROZEN 3x3 convolution of the language fusion (csrc/act_gate.hip) ---------------------------------
 * For out = mul * act(y), y = conv3x3_same([a | b], W), as mvnerf_conv3x3_nhwc wrote it, and g = dL/dout:
 *   d[n,p,c] = g * mul[n,c] * act'(y), from `out` and `mul` alone (y is not kept, nothing is divided):
 *     act(y) > 0, i.e. out and mul are both positive or both negative:  d = g * mul
 *     else, relu: d = 0;  else, elu: d = g * (out + mul)   (elu' = elu + 1);  identity: d = g * mul
 *   mul[n,c] == 0 gives an exact 0.  mul NULL means 1.  The data gradients are then mvnerf_conv3x3_nhwc of d with the transposed packs of
 *   the rows of W that a and b meet.
 * g, out, d (N, pixels_per_image, C) fp32 NHWC; d may be g (in place).  mul (N,C) or NULL.  act: 0 identity, 1 relu, 2 elu.
 * amax_out (optional): one device word the CALLER ZEROES; on return max |d| (a NaN written anywhere makes it a NaN).
 * One rounding per written operation.  No workspace, no atomics on d: two runs give the same bits.  Stream-ordered, no host read.
 * 1 <= N <= 65535, N * pixels_per_image <= 2^31 - 1: else MVNERF_E_ARG; C a multiple of 4, act in 0..2: else MVNERF_E_SHAPE; before any
 * launch.  g, out, mul, d 16-byte aligned. */
int mvnerf_act_gate_nhwc(const float* g, const float* out, const float* mul, int act, int N, long pixels_per_image, int C, float* d,
                         float* amax_out, mvnerf_stream_t stream);

/* Batch statistics of a convolution output from its tile partials (layers.py:23, 27: tf.keras BatchNormalization, training=True):
 * mean[c] and rstd[c] = 1 / sqrt(var[c] + eps) with the BIASED variance over all N h w pixels, c < Cout.  The tiles are combined with
 * Chan's pairwise update in double, in a fixed order.  Stream-ordered, no host read (the chain can be captured in a graph). */
int mvnerf_bn_finalize(const float* stats, int N, int h, int w, int Cout, double eps, float* mean, float* rstd, mvnerf_stream_t stream);

/* out = act(((y - mean[c]) * rstd[c]) * gamma[c] + beta[c] (+ skip)) over `pixels` x C fp32 NHWC elements (layers.py:23-33: the
 * normalisation, `out += skip`, relu).  skip: like y, or NULL.  act: 0 identity, 1 relu.  out may be y (in place).  amax_out (optional):
 * one device word the CALLER ZEROES; on return max |out|.  One rounding per written operation, the subtraction first.
 * C a multiple of 4; all arrays 16-byte aligned. */
int mvnerf_bn_apply_nhwc(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* skip,
                         long pixels, int C, int act, float* out, float* amax_out, mvnerf_stream_t stream);

/* ---- the transformer blocks of the ViT (layers.py:72-95 TransformerBlock) over token rows (M, C) fp32, row-major:
 * Dense layers at fp32 grade on the fp16 matrix pipe (the three-product rule of the 3x3 convolution above with one tap),
 * LayerNormalization, and self-attention in fp32.  Inference only.  The block's first norm, an eval-mode BatchNormalization over the
 * embedding axis, is mvnerf_bn_apply_nhwc with mean = the moving mean and rstd = 1 / sqrt(moving variance + eps).  Every pass is
 * stream-ordered, reads nothing on the host, has no atomics on its output and sums in a fixed order: bit-identical from run to run. */

/* Bytes of the packed stream of an (N, K) Dense weight; 0 when the shape is not accepted (K % 32, N % 64). */
size_t mvnerf_linear_packed_bytes(int K, int N);

/* weight (N, K) fp32, torch's Linear layout (the transpose of the Keras kernel) -> `packed` (16-byte aligned,
 * mvnerf_linear_packed_bytes): a 256-byte header (max |w| found on the device, the scale exponent derived from it) and the fp16 pieces
 * A0, A1, A0 / 64 in the order the kernel's K loop consumes them.  Call once per weight update. */
int mvnerf_linear_pack(const float* weight, int K, int N, void* packed, mvnerf_stream_t stream);

/* out (M, N) = epi(x (M, K) . W^T + bias).  amax_x: one device float, an UPPER BOUND of |x| (mvnerf_absmax_f32, or the amax_out of the
 * pass that wrote x); 0 means an all-zero x, a non-finite bound fills out with NaN.  bias (N) or NULL.  epi: 0 nothing more, 1 exact-erf
 * gelu, 2 `+ residual` with residual (M, N) - NULL unless epi is 2 (else MVNERF_E_ARG).  amax_out (optional): one device word the CALLER
 * ZEROES; on return max |out|.  Any M >= 1: the last tile of 32 rows is predicated, nothing is read or written past row M.
 * K a multiple of 32, N a multiple of 64, epi in 0..2: else MVNERF_E_SHAPE.  x, packed, bias, residual, out 16-byte aligned; out must
 * not overlap x. */
int mvnerf_linear_tokens(const float* x, const float* amax_x, const void* packed, const float* bias, const float* residual, long M, int K,
                         int N, int epi, float* out, float* amax_out, mvnerf_stream_t stream);

/* out = ((x - mean) * rstd) * gamma + beta per row of (M, C): mean = ref + sum(x - ref) / C with ref the row's first element, then
 * rstd = 1 / sqrt(sum((x - mean)^2) / C + eps) (biased variance), both sums in a fixed order; one rounding per written operation.  A
 * constant row gives out == beta.  out may be x (in place).  amax_out as above.  C a multiple of 4; all arrays 16-byte aligned. */
int mvnerf_layer_norm_tokens(const float* x, const float* gamma, const float* beta, long M, int C, float eps, float* out, float* amax_out,
                             mvnerf_stream_t stream);

/* qkv (B, n, 3, heads, d) fp32, the output of the QKV Dense layer as it lies -> out (B, n, heads * d) = softmax_j(q_i . k_j * scale) v_j
 * per image and head, fp32 throughout (v_mfma_f32_16x16x4_f32, the accurate expf, the row maximum subtracted first).  amax_out as above.
 * d in {16, 32, 64}, 1 <= n <= 256: else MVNERF_E_SHAPE.  qkv, out 16-byte aligned. */
int mvnerf_attention_tokens(const float* qkv, int B, int n, int heads, int d, float scale, float* out, float* amax_out,
                            mvnerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVNERF_HIP_H */
