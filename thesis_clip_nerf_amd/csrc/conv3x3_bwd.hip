// Weight (and bias) gradient of the biased, stride-1, zero-padded 3x3 convolution over NHWC fp32 maps: the backward of
// mvnerf_conv3x3_nhwc_ex for one source and an identity output, next to the data gradient, which is the forward kernel on the flipped,
// transposed weights (ops.conv3x3_pack_transposed).
//
//   dw[dy, dx, ci, co] = sum_{n, i, j} act_in(x)[n, i + dy - 1, j + dx - 1, ci] * g[n, i, j, co]        (HWIO, taps outside the image 0)
//   dbias[co]          = sum_{n, i, j} g[n, i, j, co]
//
// Nine GEMMs whose reduction runs over the PIXELS, on the fp16 matrix pipe at fp32 grade: g is cut like a weight (A0, A1, A0s), act_in(x)
// like an activation (B0, B1), each under a power-of-two scale from its device amax word, and every product block is three
// v_mfma_f32_16x16x32_f16 (mvnerf_conv.h has the arithmetic).
//
// Work split.  The 16 x 16 pixel tiles of the batch - [image][tile row][tile column] - are cut into slabs of kWgradSlabTiles.  A workgroup
// (256 threads, 4 waves) owns one slab, 32 input channels and 64 output channels, for all nine taps: wave v owns input-channel block
// v & 1 (16 channels) and output-channel blocks 2 (v >> 1), 2 (v >> 1) + 1: 18 accumulators of 4 registers.  g is the MFMA's A operand
// (rows = output channels), x its B operand (columns = input channels), so a lane ends with 4 consecutive output channels of one input
// channel and stores 16 bytes of the HWIO result.
//
// Staging.  Both operands have the pixels - the K of the MFMA - as their strided axis in memory, and a lane's fragment is 8 consecutive
// K.  A stage is half a tile, 8 rows x 16 columns = 4 k-steps of 32 pixels (two rows); k group `grp` of a k-step is row grp >> 1, columns
// 8 (grp & 1) .. + 7.  Per stage the workgroup transposes into LDS, as fp16 pieces cut once per element:
//   g   [piece A0 | A1 | A0s][output channel (64)][pixel (128)], 272 bytes per channel;
//   x   [dx (3)][piece B0 | B1][input channel (32)][halo row (10)][column (16)], 336 bytes per channel: ONE COPY PER HORIZONTAL TAP SHIFT,
//       copy dx holding column j + dx - 1 at j.  The fragment of tap (dy, dx) is then an aligned 16-byte read at halo row
//       (output row) + dy of copy dx: no unaligned LDS read, and the vertical shift is a row offset.
// A ds_read_b128 is served in groups of 16 lanes that hold all 16 channels of a block but two neighbouring k groups; the two 16-byte
// halves of a 32-byte row are therefore stored swapped for channels 4 .. 11 of every block of 16 (`wg_swap`), which puts the 16 lanes of
// a group on 16 different 16-byte bank slots (channel strides of 17 and 21 slots).  act_in is applied to x as it is staged, before the
// cut, exactly as the forward does; pixels outside the image - the halo's and a ragged tile's - are staged as zeros, so padding pixels
// count for nothing and images do not see each other.  LDS: 116 736 bytes, every byte that is read is written in the same stage.
//
// Order.  The matrix pipe sums a stage (128 pixels x 3 products) in fp32 from zero; the stage sums are added in order, in fp32, into the
// slab's registers; the slab's partial goes to `workspace` with plain 16-byte stores.  A second launch adds the slabs in order in
// double, multiplies by 2^-(ex + eg) and rounds once.  dbias comes from one more small launch in front of the combine: per (slab, 64
// channels) the pixels in a fixed order in double, rounded to an fp32 slab sum, then combined with the weights' slabs.  No atomics; the
// combine reads only what the first launches wrote; two runs give the same bits whatever the workspace held.  Stream-ordered, no host read.
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_conv.h"
#include "mvnerf_launch.h"
#include "mvnerf_mfma.h"

namespace mvnerf {

namespace {

constexpr int kWgThreads = 256;
constexpr int kWgRows = 8;                                     // output rows of a stage
constexpr int kWgHaloRows = kWgRows + 2;                       // (and 18 halo columns: three shifted copies of 16)
constexpr int kWgChunk = 32;                                   // input channels per workgroup
constexpr int kWgCout = 64;                                    // output channels per workgroup
constexpr int kWgXStride = kWgHaloRows * 32 + 16;              // 336 bytes per input channel: 21 slots of 16 bytes
constexpr int kWgXCopy = kWgChunk * kWgXStride;                // one (dx, piece)
constexpr int kWgXBytes = 6 * kWgXCopy;                        // 64 512
constexpr int kWgGStride = kWgRows * 32 + 16;                  // 272 bytes per output channel: 17 slots
constexpr int kWgGPiece = kWgCout * kWgGStride;
constexpr int kWgLdsBytes = kWgXBytes + 3 * kWgGPiece;         // 116 736
constexpr int kWgXItems = kWgHaloRows * 2 * (kWgChunk / 4);    // x staging: (halo row, half row, 4 channels) = 160 of the 256 threads
static_assert(kWgCout / 4 * kWgRows * 2 == kWgThreads, "g staging: one (pixel group of 8, 4 channels) per thread");
static_assert((kWgXStride / 16) % 2 == 1 && (kWgGStride / 16) % 2 == 1, "odd slot strides: the 16 channels of a block fall on 16 bank slots");
static_assert(kWgLdsBytes <= 160 * 1024, "one workgroup per CU");

__device__ __forceinline__ f32x4 wg_mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// 1 for channels 4 .. 11 of a block of 16: those store (and read) the two 16-byte halves of a 32-byte row swapped
__device__ __forceinline__ int wg_swap(int channel) { return (((channel & 15) + 4) >> 3) & 1; }

template <int kActIn>
__global__ __launch_bounds__(kWgThreads) void conv3x3_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ amax_x,
                                                                  const float* __restrict__ g, const float* __restrict__ amax_g, int N, int h,
                                                                  int w, int Cin, int Cout, float* __restrict__ partial, int tiles_x,
                                                                  int tiles_y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* const xl = lds;                             // [dx][piece][ci][halo row][16] fp16
    unsigned char* const gl = lds + kWgXBytes;                 // [piece][co][128] fp16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cl = lane & 15, grp = lane >> 4;
    const int cout_tiles = Cout / kWgCout, chunks = Cin / kWgChunk;
    int bid = blockIdx.x;
    const int ct = bid % cout_tiles;
    bid /= cout_tiles;
    const int cc = bid % chunks, slab = bid / chunks;
    const float max_x = *amax_x, max_g = *amax_g;
    if (!conv_amax_finite(max_x) || !conv_amax_finite(max_g)) return;      // (the same in every lane of the grid) the combine writes the NaNs
    const int ex = conv_scale_exp(max_x), eg = conv_scale_exp(max_g);
    const int per_image = tiles_x * tiles_y, tiles = N * per_image;
    const int cib = wave & 1, cop = wave >> 1;

    f32x4 total[9][2];                   // [tap][output-channel block of this wave]
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) total[t][cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // fragment addresses of this lane (without the k-step and the tap)
    const int sw = wg_swap(cl);
    const unsigned char* gfrag = gl + (16 * (2 * cop) + cl) * kWgGStride + ((grp ^ sw) << 4);
    const unsigned char* xfrag = xl + (16 * cib + cl) * kWgXStride + (grp >> 1) * 32 + (((grp & 1) ^ sw) << 4);

    const int first = slab * kWgradSlabTiles;
    const int last = first + kWgradSlabTiles < tiles ? first + kWgradSlabTiles : tiles;
    for (int tile = first; tile < last; ++tile) {
        const int n = tile / per_image, in_image = tile % per_image;
        const int y0 = (in_image / tiles_x) * kWgradTile, x0 = (in_image % tiles_x) * kWgradTile;
        for (int half = 0; half < 2; ++half) {
            const int yh = y0 + kWgRows * half;
            if (yh >= h) break;                                  // (uniform) no output pixel in this half: g is zero all over it
            __syncthreads();                                     // every wave has read the previous stage
            // ---- x: the 10 x 18 halo of 32 channels.  A thread takes 10 consecutive halo columns of one row and 4 channels (16-byte loads,
            // 8 lanes = 128 contiguous bytes of a pixel), cuts each element once and writes, per channel and piece, the 8 columns of each
            // of the three shifted copies as one 16-byte store.
            // (every load goes to a clamped, valid address and is zeroed afterwards where it lay outside: no branch between the loads, so
            // they are all in flight together; g's are issued first and land while x is cut)
            const int gq = tid & 15, pg = tid >> 4;                      // g: pixel group pg = row pg >> 1, columns 8 (pg & 1) .. + 7
            const int gy = yh + (pg >> 1);
            f32x4 gv[8];
            {
                const float* grow = g + ((size_t)n * h + (gy < h ? gy : h - 1)) * w * Cout + ct * kWgCout + 4 * gq;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ix = x0 + 8 * (pg & 1) + j;
                    gv[j] = *reinterpret_cast<const f32x4*>(grow + (size_t)(ix < w ? ix : w - 1) * Cout);
                }
            }
            if (tid < kWgXItems) {
                const int q = tid & 7, half_row = (tid >> 3) & 1, r = tid >> 4;
                const int iy = yh - 1 + r;
                const bool row_ok = iy >= 0 && iy < h;
                const float* xrow = x + ((size_t)n * h + (iy < 0 ? 0 : iy < h ? iy : h - 1)) * w * Cin + cc * kWgChunk + 4 * q;
                f32x4 v[10];
#pragma unroll
                for (int j = 0; j < 10; ++j) {
                    const int ix = x0 - 1 + 8 * half_row + j;
                    v[j] = *reinterpret_cast<const f32x4*>(xrow + (size_t)(ix < 0 ? 0 : ix < w ? ix : w - 1) * Cin);
                }
#pragma unroll
                for (int j = 0; j < 10; ++j) {
                    const int ix = x0 - 1 + 8 * half_row + j;
                    if (!(row_ok && ix >= 0 && ix < w)) v[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    unsigned b0[10], b1[10];
#pragma unroll
                    for (int j = 0; j < 10; ++j) {
                        uint16_t lo, hi;
                        conv_wgrad_cut_x(v[j][k], kActIn, ex, lo, hi);       // act_in(0) == 0: what lies outside the image stays zero
                        b0[j] = lo;
                        b1[j] = hi;
                    }
                    const int c = 4 * q + k;
                    unsigned char* dst = xl + c * kWgXStride + r * 32 + ((half_row ^ wg_swap(c)) << 4);
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {                         // copy dx holds halo column col + dx at col
                        u32x4 p0, p1;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            p0[e] = b0[dx + 2 * e] | (b0[dx + 2 * e + 1] << 16);
                            p1[e] = b1[dx + 2 * e] | (b1[dx + 2 * e + 1] << 16);
                        }
                        *reinterpret_cast<u32x4*>(dst + 2 * dx * kWgXCopy) = p0;
                        *reinterpret_cast<u32x4*>(dst + (2 * dx + 1) * kWgXCopy) = p1;
                    }
                }
            }
            // ---- g: 8 x 16 pixels of 64 channels, zero outside the image: a thread takes 8 consecutive columns and 4 channels
            {
                const int q = gq;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (!(gy < h && x0 + 8 * (pg & 1) + j < w)) gv[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    unsigned a0[8], a1[8], a0s[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        uint16_t t0, t1, t2;
                        conv_wgrad_cut_g(gv[j][k], eg, t0, t1, t2);
                        a0[j] = t0;
                        a1[j] = t1;
                        a0s[j] = t2;
                    }
                    const int c = 4 * q + k;
                    unsigned char* dst = gl + c * kWgGStride + ((pg ^ wg_swap(c)) << 4);
                    u32x4 p0, p1, p2;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        p0[e] = a0[2 * e] | (a0[2 * e + 1] << 16);
                        p1[e] = a1[2 * e] | (a1[2 * e + 1] << 16);
                        p2[e] = a0s[2 * e] | (a0s[2 * e + 1] << 16);
                    }
                    *reinterpret_cast<u32x4*>(dst) = p0;
                    *reinterpret_cast<u32x4*>(dst + kWgGPiece) = p1;
                    *reinterpret_cast<u32x4*>(dst + 2 * kWgGPiece) = p2;
                }
            }
            __syncthreads();
            // ---- 4 k-steps x 9 taps x 2 channel blocks x 3 products
            f32x4 acc[9][2];
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) acc[t][cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                u32x4 ga[2][3];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        ga[cb][p] = *reinterpret_cast<const u32x4*>(gfrag + p * kWgGPiece + cb * 16 * kWgGStride + 64 * s);
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int dy = t / 3, dx = t % 3;
                    const unsigned char* q = xfrag + 2 * dx * kWgXCopy + (2 * s + dy) * 32;
                    const u32x4 b0 = *reinterpret_cast<const u32x4*>(q);
                    const u32x4 b1 = *reinterpret_cast<const u32x4*>(q + kWgXCopy);
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) acc[t][cb] = wg_mfma(ga[cb][2], b1, acc[t][cb]);       // A0s B1
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) acc[t][cb] = wg_mfma(ga[cb][1], b0, acc[t][cb]);       // A1 B0
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) acc[t][cb] = wg_mfma(ga[cb][0], b0, acc[t][cb]);       // A0 B0
                }
            }
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) total[t][cb] = total[t][cb] + acc[t][cb];
        }
    }

    // register r of total[t][cb] is output channel 64 ct + 16 (2 cop + cb) + 4 grp + r of input channel 32 cc + 16 cib + cl
    const int ci = cc * kWgChunk + 16 * cib + cl;
    float* out = partial + (size_t)slab * 9 * Cin * Cout + (size_t)ci * Cout + ct * kWgCout + 32 * cop + 4 * grp;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) *reinterpret_cast<f32x4*>(out + (size_t)t * Cin * Cout + 16 * cb) = total[t][cb];
}

// one (slab, 64 channels): thread (channel c, group j) takes pixels j, j + 4, .. of every tile in order, in double; the four groups in order
__global__ __launch_bounds__(kWgThreads) void conv3x3_dbias_kernel(const float* __restrict__ g, const float* __restrict__ amax_x,
                                                                  const float* __restrict__ amax_g, int N, int h, int w, int Cout,
                                                                  float* __restrict__ partial, int tiles_x, int tiles_y) {
    __shared__ double part[4][kWgCout];
    if (!conv_amax_finite(*amax_x) || !conv_amax_finite(*amax_g)) return;
    const int c = threadIdx.x & (kWgCout - 1), j = threadIdx.x >> 6;
    const int cout_tiles = Cout / kWgCout, ct = blockIdx.x % cout_tiles, slab = blockIdx.x / cout_tiles;
    const int per_image = tiles_x * tiles_y, tiles = N * per_image;
    const int first = slab * kWgradSlabTiles;
    const int last = first + kWgradSlabTiles < tiles ? first + kWgradSlabTiles : tiles;
    double sum = 0.0;
    for (int tile = first; tile < last; ++tile) {
        const int n = tile / per_image, in_image = tile % per_image;
        const int y0 = (in_image / tiles_x) * kWgradTile, x0 = (in_image % tiles_x) * kWgradTile;
        for (int i = j; i < kWgradTile * kWgradTile; i += 4) {
            const int iy = y0 + (i >> 4), ix = x0 + (i & 15);
            if (iy < h && ix < w) sum = sum + (double)g[(((size_t)n * h + iy) * w + ix) * Cout + ct * kWgCout + c];
        }
    }
    part[j][c] = sum;
    __syncthreads();
    if (j == 0) partial[(size_t)slab * Cout + ct * kWgCout + c] = (float)(((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]);
}

// one thread per weight (then per bias): the slabs in order, in double
__global__ __launch_bounds__(256) void conv3x3_wgrad_combine_kernel(const float* __restrict__ partial, const float* __restrict__ bias_partial,
                                                                   const float* __restrict__ amax_x, const float* __restrict__ amax_g, long weights,
                                                                   int Cout, int slabs, float* __restrict__ dw, float* __restrict__ dbias) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= weights + (dbias ? Cout : 0)) return;
    const float max_x = *amax_x, max_g = *amax_g;
    const bool is_w = idx < weights;
    const bool skip = !conv_amax_finite(max_x) || !conv_amax_finite(max_g) || max_g == 0.0f || (is_w && max_x == 0.0f);
    const float* src = is_w ? partial + idx : bias_partial + (idx - weights);
    const long stride = is_w ? weights : Cout;
    double sum = 0.0;
    if (!skip)
        for (int s = 0; s < slabs; ++s) sum = sum + (double)src[(size_t)s * stride];
    if (is_w)
        dw[idx] = conv_wgrad_finish(sum, max_x, max_g);
    else
        dbias[idx - weights] = conv_dbias_finish(sum, max_x, max_g);
}

bool wgrad_shape_ok(int N, int h, int w, int Cin, int Cout) {
    if (N <= 0 || h <= 0 || w <= 0 || Cin < kWgChunk || Cin % kWgChunk || Cout < kWgCout || Cout % kWgCout) return false;
    const long blocks = conv_wgrad_slabs(N, h, w) * (Cin / kWgChunk) * (Cout / kWgCout);
    return (long)N * h * w <= 0x7fffffffL && blocks <= 0x7fffffffL && 9L * Cin * Cout + Cout <= 0x7fffffffL;
}

}  // namespace

}  // namespace mvnerf

extern "C" {

int mvnerf_conv3x3_wgrad_slab_pixels(void) { return mvnerf::kWgradSlabPixels; }

size_t mvnerf_conv3x3_wgrad_workspace_bytes(int N, int h, int w, int Cin, int Cout) {
    using namespace mvnerf;
    if (!wgrad_shape_ok(N, h, w, Cin, Cout)) return 0;
    return (size_t)conv_wgrad_slabs(N, h, w) * (9 * (size_t)Cin * Cout + Cout) * sizeof(float);
}

int mvnerf_conv3x3_wgrad_nhwc(const float* x, const float* amax_x, int act_in, const float* g, const float* amax_g, int N, int h, int w, int Cin,
                              int Cout, float* dw_hwio, float* dbias, void* workspace, mvnerf_stream_t stream) {
    using namespace mvnerf;
    const char* who = "mvnerf_conv3x3_wgrad_nhwc";
    if (!x || !amax_x || !g || !amax_g || !dw_hwio || !workspace)
        return api_fail(MVNERF_E_ARG, "%s: null pointer (%s)", who,
                        !x ? "x" : !amax_x ? "amax_x" : !g ? "g" : !amax_g ? "amax_g" : !dw_hwio ? "dw_hwio" : "workspace");
    if (N <= 0 || h <= 0 || w <= 0) return api_fail(MVNERF_E_ARG, "%s: N=%d h=%d w=%d", who, N, h, w);
    if (Cin < kWgChunk || Cin % kWgChunk) return api_fail(MVNERF_E_SHAPE, "%s: Cin=%d (a multiple of 32, at least 32)", who, Cin);
    if (Cout < kWgCout || Cout % kWgCout) return api_fail(MVNERF_E_SHAPE, "%s: Cout=%d (a multiple of 64, at least 64)", who, Cout);
    if (act_in < 0 || act_in > 2) return api_fail(MVNERF_E_SHAPE, "%s: act_in=%d (0 identity, 1 relu, 2 elu)", who, act_in);
    if (!wgrad_shape_ok(N, h, w, Cin, Cout))
        return api_fail(MVNERF_E_SHAPE, "%s: N=%d h=%d w=%d Cin=%d Cout=%d (pixels, workgroups and weights at most 2^31 - 1 each)", who, N, h, w,
                        Cin, Cout);
    if (!aligned16(x) || !aligned16(g) || !aligned16(dw_hwio) || !aligned16(dbias) || !aligned16(workspace))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 16-byte aligned", who,
                        !aligned16(x) ? "x" : !aligned16(g) ? "g" : !aligned16(dw_hwio) ? "dw_hwio" : !aligned16(dbias) ? "dbias" : "workspace");
    if (!aligned4(amax_x) || !aligned4(amax_g))
        return api_fail(MVNERF_E_ALIGN, "%s: %s must be 4-byte aligned", who, !aligned4(amax_x) ? "amax_x" : "amax_g");
    static DeviceSetup setup;
    MV_HIP(device_setup(setup, {{conv3x3_wgrad_kernel<0>, kWgLdsBytes}, {conv3x3_wgrad_kernel<1>, kWgLdsBytes},
                                {conv3x3_wgrad_kernel<2>, kWgLdsBytes}}), who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int tiles_x = (w + kWgradTile - 1) / kWgradTile, tiles_y = (h + kWgradTile - 1) / kWgradTile;
    const int slabs = (int)conv_wgrad_slabs(N, h, w);
    const long weights = 9L * Cin * Cout;
    float* partial = static_cast<float*>(workspace);
    float* bias_partial = partial + (size_t)slabs * weights;
    auto* kernel = act_in == 0 ? conv3x3_wgrad_kernel<0> : act_in == 1 ? conv3x3_wgrad_kernel<1> : conv3x3_wgrad_kernel<2>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((long)slabs * (Cin / kWgChunk) * (Cout / kWgCout))), dim3(kWgThreads), kWgLdsBytes, st, x, amax_x, g,
                       amax_g, N, h, w, Cin, Cout, partial, tiles_x, tiles_y);
    MV_HIP(hipGetLastError(), who);
    if (dbias) {
        hipLaunchKernelGGL(conv3x3_dbias_kernel, dim3((unsigned)(slabs * (Cout / kWgCout))), dim3(kWgThreads), 0, st, g, amax_x, amax_g, N, h, w, Cout,
                           bias_partial, tiles_x, tiles_y);
        MV_HIP(hipGetLastError(), who);
    }
    const long outputs = weights + (dbias ? Cout : 0);
    hipLaunchKernelGGL(conv3x3_wgrad_combine_kernel, dim3((unsigned)((outputs + 255) / 256)), dim3(256), 0, st, partial, bias_partial, amax_x, amax_g,
                       weights, Cout, slabs, dw_hwio, dbias);
    return hip_status(hipGetLastError(), who);
}

}  // extern "C"
