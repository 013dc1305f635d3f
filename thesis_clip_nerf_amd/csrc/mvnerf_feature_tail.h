// Arithmetic and index rules of the backward pass of the producers' tail (feature_tail_bwd.hip), as plain inline code for
// host and device: tests/cpu_feature_tail_bwd builds this file with the host compiler and compares it bit for bit with the NumPy
// restatement of tests/feature_tail_bwd_ref.py.
//
//   forward     out = bilinear_x2( act(X) . W ),  X = [a | b] (N,h,w,Ca+Cb),  W (Ca+Cb, 256)                 (feature_tail.hip)
//   adjoint     g_low[n,y,x,c] = sum_{Y,X'} cy(Y,y) cx(X',x) g[n,Y,X',c]
//   data        dX[n,y,x,k]    = act'(X[n,y,x,k]) * sum_c g_low[n,y,x,c] W[k,c]
//
//   coefficient  Output index O of an axis with n low samples blends low indices (O - 1) >> 1 and ((O - 1) >> 1) + 1, both clamped into
//                [0, n - 1], with (3/4, 1/4) for odd O and (1/4, 3/4) for even O.  c(O, l) is the sum of the taps of O that land on l: the
//                two clamped taps of O = 0 (and of O = 2n - 1) fold onto one low index and give 1/4 + 3/4 = 1, exactly.
//   terms        Low index l receives the outputs 2l - 1 + t, t = 0..3, that exist (0 <= O < 2n); each of them has a non-zero coefficient.
//   order        rows first: v(X') = sum_t cy_t g[Y_t, X'], from +0, t ascending; then g_low = sum_u cx_u v(X'_u), from +0, u ascending.
//                Each product and each addition rounds once (-ffp-contract=off); 1/4 and 1 are exact factors.  A term that does not
//                exist is not formed, so a NaN in g reaches only the low pixels it has a coefficient for.
//   act'         identity d; relu x > 0 ? d : 0; elu x > 0 ? d : d expf(x).  A masked relu element is 0 whatever d is.
//   tiling       kFtbTileH x kFtbTileW = 8 x 16 low pixels per workgroup, tiles [image][tile row][tile column], no overlap; a ragged tile
//                forms and stores only the pixels inside the image.
#pragma once

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MVF_HD __host__ __device__ inline
#else
#define MVF_HD inline
#endif

namespace mvnerf {

constexpr int kFtbOut = 256;                         // channels of g and of g_low: the forward's filters
constexpr int kFtbTileH = 8, kFtbTileW = 16;         // low pixels of a tile
constexpr int kFtbTilePix = kFtbTileH * kFtbTileW;   // 128 = 4 MFMA row blocks

// c(O, l): the weight with which output index O of an axis of n low samples reads low index l (0 where it does not)
MVF_HD float ftb_coef(int O, int l, int n) {
    const int t0 = (O - 1) >> 1, t1 = t0 + 1;                      // (arithmetic shift: O = 0 starts at -1)
    const int l0 = t0 < 0 ? 0 : t0, l1 = t1 > n - 1 ? n - 1 : t1;
    const float w0 = (O & 1) ? 0.75f : 0.25f, w1 = (O & 1) ? 0.25f : 0.75f;
    float c = 0.0f;
    if (l0 == l) c = c + w0;
    if (l1 == l) c = c + w1;
    return c;
}

// The <= 4 outputs that feed low index l of an axis with n low samples: O = first + t where on[t], with coefficient c[t].
struct FtbTaps {
    int first;
    float c[4];
    bool on[4];
};

MVF_HD FtbTaps ftb_taps(int l, int n) {
    FtbTaps taps;
    taps.first = 2 * l - 1;
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < 4; ++t) {
        const int O = taps.first + t;
        taps.on[t] = O >= 0 && O < 2 * n;
        taps.c[t] = taps.on[t] ? ftb_coef(O, l, n) : 0.0f;
    }
    return taps;
}

// one more term of an adjoint sum: the product rounds, then the addition (T: float, or a vector of floats on the device)
template <class T>
MVF_HD T ftb_add(T acc, float c, T g) {
    const T term = g * c;
    return acc + term;
}

MVF_HD float ftb_act_grad(float x, float d, int act) {
    if (act == 1) return x > 0.0f ? d : 0.0f;
    if (act == 2) return x > 0.0f ? d : d * expf(x);
    return d;
}

// ---- tiling ---------------------------------------------------------------------------------------------------------------------------
MVF_HD int ftb_tiles_y(int h) { return (h + kFtbTileH - 1) / kFtbTileH; }
MVF_HD int ftb_tiles_x(int w) { return (w + kFtbTileW - 1) / kFtbTileW; }
MVF_HD long ftb_tiles(int N, int h, int w) { return (long)N * ftb_tiles_y(h) * ftb_tiles_x(w); }

struct FtbTile {
    int n, y0, x0;       // image, first low row and column
};

MVF_HD FtbTile ftb_tile(long tile, int h, int w) {
    const int tiles_x = ftb_tiles_x(w), tiles_y = ftb_tiles_y(h);
    FtbTile t;
    t.x0 = (int)(tile % tiles_x) * kFtbTileW;
    tile /= tiles_x;
    t.y0 = (int)(tile % tiles_y) * kFtbTileH;
    t.n = (int)(tile / tiles_y);
    return t;
}

// pixel p (0..127) of a tile: row p / 16, column p % 16; inside the image?
MVF_HD int ftb_pixel_y(FtbTile t, int p) { return t.y0 + p / kFtbTileW; }
MVF_HD int ftb_pixel_x(FtbTile t, int p) { return t.x0 + p % kFtbTileW; }
MVF_HD bool ftb_inside(int y, int x, int h, int w) { return y < h && x < w; }

// element offsets (in floats) of a low pixel (channel stride C) and of an output pixel of g
MVF_HD size_t ftb_low_offset(int n, int y, int x, int h, int w, int C) { return (((size_t)n * h + y) * w + x) * C; }
MVF_HD size_t ftb_out_offset(int n, int Y, int X, int h, int w) { return (((size_t)n * (2 * h) + Y) * (2 * w) + X) * kFtbOut; }

// The tile pixel that accumulator register r of row block m holds on lane half `half` of the 32x32x2 fp32 MFMA (its 32 lanes j are 32
// consecutive input channels)
MVF_HD int ftb_acc_pixel(int m, int r, int half) { return 32 * m + (r & 3) + 8 * (r >> 2) + 4 * half; }

}  // namespace mvnerf
