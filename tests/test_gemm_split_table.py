"""The split counts tests/gemm_cases.py names, checked through the three *_scratch_bytes functions (host arithmetic, no GPU): a later change
of the split rule cannot move a case of tests/test_gpu_gemm_exact.py off its edge unseen."""
import pytest

from tests import gemm_cases as G
from thesis_clip_nerf_amd import _lib


@pytest.mark.parametrize('shape,splits', G.NT)
def test_gemm_nt_split_count(shape, splits):
    m, n, k = shape
    nbytes = int(_lib.lib().mvnerf_gemm_nt_scratch_bytes(m, n, k))
    assert nbytes == (0 if splits == 1 else 4 * m * n * splits)
    assert G.nt_splits(m, n, k) == splits


@pytest.mark.parametrize('shape,splits', G.TN)
def test_gemm_tn_split_count(shape, splits):
    m, n, k = shape
    nbytes = int(_lib.lib().mvnerf_gemm_tn_scratch_bytes(m, n, k))
    assert nbytes == (0 if splits == 1 else 4 * n * k * splits)
    assert G.tn_splits(m, n, k) == splits


@pytest.mark.parametrize('with_colsum', [False, True])
@pytest.mark.parametrize('shape,splits', G.BATCHED)
def test_gemm_tn_batched_split_count(shape, splits, with_colsum):
    m, n, k, batch = shape
    nbytes = int(_lib.lib().mvnerf_gemm_tn_batched_scratch_bytes(m, n, k, batch, int(with_colsum)))
    assert nbytes == (0 if splits == 1 else 4 * batch * (n * k + (n if with_colsum else 0)) * splits)
    assert G.batched_splits(m, n, k, batch, with_colsum) == splits


def test_the_table_covers_the_reduce_boundaries_and_both_ends():
    for table in (G.NT, G.TN, G.BATCHED):
        counts = {s for _, s in table}
        assert {1, 2, 17, 33} <= counts
    assert {16, 17, 32, 33, 48, 49, 64, 512} <= {s for _, s in G.NT}
    assert all(k % 8 == 0 and k // 8 >= s for (_, _, k), s in G.NT)              # every range has at least one k-step
    assert all(m % 8 == 0 and m // 8 >= s for (m, _, _), s in G.TN)
    assert any((k // 8) % s for (_, _, k), s in G.NT if s > 1)                   # a split count that does not divide the step count
    assert any((m // 32) * (n // 64) % 4 for (m, n, _), s in G.NT)               # a tile count that is no multiple of the 4 waves
    assert any((m // 32) * (n // 64) >= 1024 for (m, n, _), s in G.NT)
