// C entry points over the bias / act_in / batch-statistics part of thesis_clip_nerf_amd/csrc/mvnerf_conv.h for tests/test_bn_conv_cpu.py
// (arrays in, arrays out).  The tile statistics walk a tile in the kernel's order (csrc/conv3x3.hip): a channel's 256 pixels lie in 4
// registers (rows 4 wave + nb) x 16 lanes (columns) x 4 waves; registers first, an xor butterfly over the 16 lanes, the waves in order.
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_conv.h"

using namespace mvnerf;

namespace {

// sum over one tile of term(value) for the real pixels, in the kernel's order; y points at channel c of image n
template <class Term>
float tile_sum(const float* y, int h, int w, int C, int y0, int x0, Term term) {
    float waves[4];
    for (int wave = 0; wave < 4; ++wave) {
        float lane[16];
        for (int col = 0; col < 16; ++col) {
            float s = 0.0f;
            for (int nb = 0; nb < 4; ++nb) {
                const int py = y0 + 4 * wave + nb, px = x0 + col;
                const bool real = py < h && px < w;
                s = s + (real ? term(y[((size_t)py * w + px) * C]) : 0.0f);
            }
            lane[col] = s;
        }
        for (int mask = 1; mask < 16; mask <<= 1) {
            float next[16];
            for (int col = 0; col < 16; ++col) next[col] = lane[col] + lane[col ^ mask];
            for (int col = 0; col < 16; ++col) lane[col] = next[col];
        }
        waves[wave] = lane[0];
    }
    return ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

}  // namespace

extern "C" {

void bn_cpu_act_in(const float* x, long n, int act_in, float* out) {
    for (long i = 0; i < n; ++i) out[i] = conv_act_f(x[i], act_in);
}

// sum (rows, C) + bias (C) -> act(sum + bias)
void bn_cpu_bias_act(const float* sum, const float* bias, long rows, int C, int act, float* out) {
    for (long i = 0; i < rows; ++i)
        for (int c = 0; c < C; ++c) out[i * C + c] = conv_bias_act(sum[i * C + c], bias[c], act);
}

// y (N,h,w,C) -> stats [channel tile][image][tile row][tile column][mean | M2][64], the layout mvnerf_conv3x3_nhwc_ex writes
void bn_cpu_tile_stats(const float* y, int N, int h, int w, int C, float* stats) {
    const int tiles_x = (w + kBnTile - 1) / kBnTile, tiles_y = (h + kBnTile - 1) / kBnTile;
    for (int ct = 0; ct < C / kBnCout; ++ct)
        for (int n = 0; n < N; ++n)
            for (int ty = 0; ty < tiles_y; ++ty)
                for (int tx = 0; tx < tiles_x; ++tx) {
                    float* slot = stats + ((((size_t)ct * N + n) * tiles_y + ty) * tiles_x + tx) * 2 * kBnCout;
                    const int count = conv_tile_pixels(h, w, ty, tx, kBnTile), y0 = ty * kBnTile, x0 = tx * kBnTile;
                    for (int c = 0; c < kBnCout; ++c) {
                        const float* src = y + (size_t)n * h * w * C + ct * kBnCout + c;
                        const float ref = src[((size_t)y0 * w + x0) * C];
                        const float mean = bn_tile_mean(ref, tile_sum(src, h, w, C, y0, x0, [&](float v) { return v - ref; }), count);
                        slot[c] = mean;
                        slot[kBnCout + c] = tile_sum(src, h, w, C, y0, x0, [&](float v) { return bn_sq_dev(v, mean); });
                    }
                }
}

// the finalize pass: per channel 16 runs of consecutive tiles, then the runs in order
void bn_cpu_finalize(const float* stats, int N, int h, int w, int C, double eps, float* mean, float* rstd) {
    const size_t tiles = (size_t)N * ((h + kBnTile - 1) / kBnTile) * ((w + kBnTile - 1) / kBnTile);
    for (int ch = 0; ch < C; ++ch) {
        const float* src = stats + (ch / kBnCout) * tiles * 2 * kBnCout + ch % kBnCout;
        BnMoments acc = bn_combine_run(src, 0, N, h, w);
        for (int r = 1; r < kBnRuns; ++r) acc = bn_chan_combine(acc, bn_combine_run(src, r, N, h, w));
        mean[ch] = (float)acc.mean;
        rstd[ch] = bn_rstd(acc, eps);
    }
}

void bn_cpu_apply(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* skip, long pixels, int C,
                  int act, float* out) {
    for (long i = 0; i < pixels; ++i)
        for (int c = 0; c < C; ++c)
            out[i * C + c] = bn_apply_one(y[i * C + c], mean[c], rstd[c], gamma[c], beta[c], skip != nullptr, skip ? skip[i * C + c] : 0.0f, act);
}

}  // extern "C"
