// C entry points over thesis_clip_nerf_amd/csrc/mvnerf_feature_tail.h for tests/test_feature_tail_bwd_cpu.py.  The walks below follow
// feature_tail_bwd.hip loop for loop - tile, wave = low row, the 16 pixels of the row with the two carried columns; then the accumulator
// registers of the epilogue - with every index taken from the header's functions.
#include "../../thesis_clip_nerf_amd/csrc/mvnerf_feature_tail.h"

using namespace mvnerf;

namespace {

struct Bounds {
    size_t g_floats;
    long bad;          // reads of g that would leave the array
};

// v(X): the rows of output column X that feed the low row with taps ty, one channel
float column(const float* g, int n, const FtbTaps& ty, int X, int h, int w, int c, Bounds& bounds) {
    float acc = 0.0f;
    for (int t = 0; t < 4; ++t) {
        if (!ty.on[t]) continue;
        const size_t at = ftb_out_offset(n, ty.first + t, X, h, w);
        if (X < 0 || X >= 2 * w || at + kFtbOut > bounds.g_floats) {
            ++bounds.bad;
            continue;
        }
        acc = ftb_add(acc, ty.c[t], g ? g[at + c] : 0.0f);
    }
    return acc;
}

}  // namespace

extern "C" {

int ftb_cpu_tile_h() { return kFtbTileH; }
int ftb_cpu_tile_w() { return kFtbTileW; }
long ftb_cpu_tiles(int N, int h, int w) { return ftb_tiles(N, h, w); }
float ftb_cpu_coef(int O, int l, int n) { return ftb_coef(O, l, n); }

// the taps of low index l: first output index, 4 coefficients, 4 flags
int ftb_cpu_taps(int l, int n, float* c, int* on) {
    const FtbTaps taps = ftb_taps(l, n);
    for (int t = 0; t < 4; ++t) {
        c[t] = taps.c[t];
        on[t] = taps.on[t];
    }
    return taps.first;
}

void ftb_cpu_act_grad(const float* x, const float* d, long n, int act, float* out) {
    for (long i = 0; i < n; ++i) out[i] = ftb_act_grad(x[i], d[i], act);
}

// The gather of the whole map in the kernel's walk.  g (N,2h,2w,256) or NULL (indices only); g_low (N,h,w,256) or NULL; writes (N,h,w)
// counts the times a low pixel is written.  Returns the number of reads of g outside its array.
long ftb_cpu_adjoint(const float* g, int N, int h, int w, float* g_low, int* writes) {
    Bounds bounds = {(size_t)N * (2 * h) * (2 * w) * kFtbOut, 0};
    const int channels = g ? kFtbOut : 1;
    const long tiles = ftb_tiles(N, h, w);
    for (long t = 0; t < tiles; ++t) {
        const FtbTile tile = ftb_tile(t, h, w);
        for (int wave = 0; wave < kFtbTileH; ++wave) {
            const int y = tile.y0 + wave;
            if (y >= h) continue;
            const FtbTaps ty = ftb_taps(y, h);
            for (int c = 0; c < channels; ++c) {
                float v0 = 0.0f, v1 = 0.0f;
                if (tile.x0 > 0) {
                    v0 = column(g, tile.n, ty, 2 * tile.x0 - 1, h, w, c, bounds);
                    v1 = column(g, tile.n, ty, 2 * tile.x0, h, w, c, bounds);
                } else {
                    v1 = column(g, tile.n, ty, 0, h, w, c, bounds);
                }
                for (int q = 0; q < kFtbTileW; ++q) {
                    const int x = tile.x0 + q;
                    if (x >= w) continue;
                    const FtbTaps tx = ftb_taps(x, w);
                    float v2 = 0.0f, v3 = 0.0f;
                    if (tx.on[2]) v2 = column(g, tile.n, ty, tx.first + 2, h, w, c, bounds);
                    if (tx.on[3]) v3 = column(g, tile.n, ty, tx.first + 3, h, w, c, bounds);
                    float acc = 0.0f;
                    if (tx.on[0]) acc = ftb_add(acc, tx.c[0], v0);
                    if (tx.on[1]) acc = ftb_add(acc, tx.c[1], v1);
                    if (tx.on[2]) acc = ftb_add(acc, tx.c[2], v2);
                    if (tx.on[3]) acc = ftb_add(acc, tx.c[3], v3);
                    const size_t at = ftb_low_offset(tile.n, y, x, h, w, 1);
                    if (g_low) g_low[at * kFtbOut + c] = acc;
                    if (writes && c == 0) ++writes[at];
                    v0 = v2;
                    v1 = v3;
                }
            }
        }
    }
    return bounds.bad;
}

// The epilogue's walk for one input channel k of `a` (C = Ca) or `b` (C = Cb): stores (N,h,w) counts the stores per low pixel.  Returns
// the number of accesses (the read of X and the store are at the same offset) outside the (N,h,w,C) array.
long ftb_cpu_epilogue(int N, int h, int w, int C, int k, int* stores) {
    const size_t floats = (size_t)N * h * w * C;
    long bad = 0;
    const long tiles = ftb_tiles(N, h, w);
    for (long t = 0; t < tiles; ++t) {
        const FtbTile tile = ftb_tile(t, h, w);
        for (int half = 0; half < 2; ++half) {
            const int x_lane = tile.x0 + 4 * half;
            const size_t first = ftb_low_offset(tile.n, tile.y0, 0, h, w, C) + k;
            for (int m = 0; m < 4; ++m)
                for (int r = 0; r < 16; ++r) {
                    const int i = ftb_acc_pixel(m, r, 0) / kFtbTileW, x = x_lane + ftb_acc_pixel(m, r, 0) % kFtbTileW;
                    if (!ftb_inside(tile.y0 + i, x, h, w)) continue;
                    const size_t at = first + ((size_t)i * w + x) * C;
                    if (at >= floats) {
                        ++bad;
                        continue;
                    }
                    // the same pixel by the register's own formula
                    const int p = ftb_acc_pixel(m, r, half);
                    if (ftb_low_offset(tile.n, ftb_pixel_y(tile, p), ftb_pixel_x(tile, p), h, w, C) + k != at) ++bad;
                    ++stores[at / C];
                }
        }
    }
    return bad;
}

}  // extern "C"
