"""The shapes of tests/test_gpu_gemm_exact.py with the split count each is meant to hit, and how the real count is read off the library's
scratch sizes (host arithmetic: tests/test_gemm_split_table.py checks the table without a GPU).  A helper for the tests, not a conftest.

gemm_reduce_kernel (csrc/gemm_ops.hip) walks the partials in strides of 32 with a 16-way tail, so its boundaries lie at 16 / 17, 32 / 33 and
48 / 49 splits; 512 is the cap; a range of one k-step re-reads that step as its own prefetch; 1024 tiles switch the split off."""
from thesis_clip_nerf_amd import _lib

# (M, N, K) -> splits: c (M, N) = a (M, K) bt (N, K)^T, one wave per 32 x 64 tile, K in steps of 8
NT = [
    ((32, 64, 8), 1),               # one k-step, one wave of four
    ((32, 64, 184), 2),             # 23 steps over 2 ranges: 11 + 12
    ((32, 64, 1032), 16), ((32, 64, 1096), 17),               # reduce: first stride boundary
    ((32, 64, 2056), 32), ((32, 64, 2120), 33),               # second
    ((32, 64, 3080), 48), ((32, 64, 3144), 49),               # third
    ((32, 64, 32776), 512),         # the cap, 4097 steps
    ((160, 64, 4104), 64),          # 5 tiles: not a multiple of the 4 waves of a workgroup
    ((96, 2688, 1096), 17),         # 126 tiles, split
    ((32768, 64, 8), 1), ((1024, 2048, 16), 1),               # 1024 tiles: the no-split threshold
]
# (M, N, K) -> splits: c (N, K) = g (M, N)^T a (M, K), one wave per 32 x 64 tile, M contracted in steps of 8
TN = [((8, 32, 64), 1), ((136, 32, 64), 2), ((1096, 32, 64), 17), ((2120, 32, 64), 33), ((32776, 32, 64), 512), ((4104, 160, 64), 64),
      ((16, 1024, 2048), 1)]
# (M, N, K, batch) -> splits
BATCHED = [((8, 64, 128, 4), 1), ((64, 64, 128, 4), 1), ((136, 64, 64, 2), 2), ((1096, 64, 256, 1), 17), ((2120, 32, 64, 1), 33)]


def nt_splits(m, n, k):
    """Bytes of scratch over the bytes of one partial; 0 bytes means no split."""
    return max(1, int(_lib.lib().mvnerf_gemm_nt_scratch_bytes(m, n, k)) // (4 * m * n))


def tn_splits(m, n, k):
    return max(1, int(_lib.lib().mvnerf_gemm_tn_scratch_bytes(m, n, k)) // (4 * n * k))


def batched_splits(m, n, k, batch, with_colsum):
    return max(1, int(_lib.lib().mvnerf_gemm_tn_batched_scratch_bytes(m, n, k, batch, int(with_colsum))) // (4 * batch * (n * k + (n if with_colsum else 0))))
