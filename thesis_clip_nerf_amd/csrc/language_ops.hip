// The losses of LanguageNeRF.train_step (src/lib/lmvnerf/model_v4.py:277-318) with their cotangents, one launch each:
//
//   landscape_loss : predicted success (B, np) and its label -> the loss (mean over the batch) and weight * d loss / d success
//                    (kl_divergence after a softmax, or cross_entropy from logits: train_language.py:40-63).
//   cosine_loss    : d prediction / d pose (rows, 3|4|6) and its label -> -mean cosine similarity and scale * its derivative; the 6d form is
//                    the two 3-halves taken separately and added (model_v4.py:306-314).
//
// The math per row is mvnerf_language.h (also built for the host by tests/cpu_language).  Both are one workgroup: the rows are a few
// hundred floats; each thread walks its rows in order and a fixed LDS tree adds the threads (no atomics: the same bits from run to run).
#include <hip/hip_runtime.h>

#include "mvnerf_api.h"
#include "mvnerf_language.h"

namespace mvnerf {

namespace {

constexpr int kLossThreads = 256;

// the block's sum of v in a fixed order; every thread gets it
__device__ float block_sum(float v, float* lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = kLossThreads / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    const float r = lds[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kLossThreads) void landscape_loss_kernel(const float* __restrict__ y, const float* __restrict__ label, int B, int np,
                                                                      int kind, float coef, float* __restrict__ g_y, float* __restrict__ loss) {
    __shared__ float lds[kLossThreads];
    float acc = 0.0f;
    for (int b = threadIdx.x; b < B; b += kLossThreads) {
        float* g = g_y + (long)b * np;
        acc += language::landscape_row(kind, y + (long)b * np, label + (long)b * np, np, g);
        for (int j = 0; j < np; ++j) g[j] = coef * g[j];
    }
    const float total = block_sum(acc, lds);
    if (threadIdx.x == 0) loss[0] = total / (float)B;
}

__global__ __launch_bounds__(kLossThreads) void cosine_loss_kernel(const float* __restrict__ x, const float* __restrict__ label, long rows, int dim,
                                                                   float coef, float* __restrict__ g_x, float* __restrict__ loss) {
    __shared__ float lds[kLossThreads];
    const int halves = dim == 6 ? 2 : 1, d = dim == 6 ? 3 : dim;
    float acc = 0.0f;
    for (long r = threadIdx.x; r < rows; r += kLossThreads)
        for (int h = 0; h < halves; ++h) {
            float xv[4], lv[4], g[4];
            const long at = r * dim + 3 * h;
            for (int i = 0; i < d; ++i) { xv[i] = x[at + i]; lv[i] = label[at + i]; }
            acc += language::cosine_row(xv, lv, d, g);
            for (int i = 0; i < d; ++i) g_x[at + i] = coef * g[i];
        }
    const float total = block_sum(acc, lds);
    if (threadIdx.x == 0) loss[0] = -(total / (float)rows);
}

}  // namespace

}  // namespace mvnerf

extern "C" {

using mvnerf::aligned4;
using mvnerf::hip_status;

int mvnerf_landscape_loss(const float* y, const float* label, int B, int np, int kind, float weight, float* g_y, float* loss,
                          mvnerf_stream_t stream) {
    if (!y || !label || !g_y || !loss) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_landscape_loss: null pointer");
    if (B <= 0 || np <= 0) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_landscape_loss: B=%d np=%d", B, np);
    if (kind != MVNERF_LOSS_KL_DIVERGENCE && kind != MVNERF_LOSS_CROSS_ENTROPY)
        return mvnerf::api_fail(MVNERF_E_SHAPE, "mvnerf_landscape_loss: kind=%d (0 kl_divergence, 1 cross_entropy)", kind);
    if (!aligned4(y) || !aligned4(label) || !aligned4(g_y) || !aligned4(loss)) return mvnerf::api_fail(MVNERF_E_ALIGN, "mvnerf_landscape_loss: buffers must be 4-byte aligned");
    // kl_divergence is one loss per batch element, summed by the step; cross_entropy is their mean
    const float coef = kind == MVNERF_LOSS_CROSS_ENTROPY ? weight / (float)B : weight;
    hipLaunchKernelGGL(mvnerf::landscape_loss_kernel, dim3(1), dim3(mvnerf::kLossThreads), 0, static_cast<hipStream_t>(stream), y, label, B, np, kind,
                       coef, g_y, loss);
    return hip_status(hipGetLastError(), "mvnerf_landscape_loss");
}

int mvnerf_cosine_loss(const float* x, const float* label, long rows, int dim, float scale, float* g_x, float* loss, mvnerf_stream_t stream) {
    if (!x || !label || !g_x || !loss) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_cosine_loss: null pointer");
    if (rows <= 0) return mvnerf::api_fail(MVNERF_E_ARG, "mvnerf_cosine_loss: rows=%ld", rows);
    if (dim != 3 && dim != 4 && dim != 6) return mvnerf::api_fail(MVNERF_E_SHAPE, "mvnerf_cosine_loss: dim=%d (3, 4, or 6 = two halves of 3)", dim);
    if (!aligned4(x) || !aligned4(label) || !aligned4(g_x) || !aligned4(loss)) return mvnerf::api_fail(MVNERF_E_ALIGN, "mvnerf_cosine_loss: buffers must be 4-byte aligned");
    hipLaunchKernelGGL(mvnerf::cosine_loss_kernel, dim3(1), dim3(mvnerf::kLossThreads), 0, static_cast<hipStream_t>(stream), x, label, rows, dim,
                       -(scale / (float)rows), g_x, loss);
    return hip_status(hipGetLastError(), "mvnerf_cosine_loss");
}

}  // extern "C"
