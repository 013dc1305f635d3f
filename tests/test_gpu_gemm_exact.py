"""mvnerf_gemm_nt / _tn / _tn_batched (csrc/gemm_ops.hip) held bit-exact.  The operands are integers from [-8, 8] stored as float32: every
product is at most 64 in magnitude and every partial sum stays below 2^24, so float64 and every fp32 summation order give the same number
and the result must equal the float64 product bit for bit, whatever the split.  No tolerance anywhere in this file.

Each case names the split count it is meant to hit (tests/gemm_cases.py; the edges of gemm_reduce_kernel's strides of 32 with a 16-way
tail, a single k-step, a split that does not divide the step count, a tile count that is no multiple of 4, the no-split threshold) and
asserts that the library's scratch size still gives that count."""
import functools

import pytest
import torch

from tests import gemm_cases as G
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT = 2 ** 24
NAN_BITS = 0x7FC00000
SENTINEL = -12345.0


def ints(shape, seed):
    """Integers drawn uniformly from [-8, 8] as float32, on the CPU."""
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float()


def exact(got, want):
    """got (device, float32) equals want (CPU, float64) bit for bit; the premise of exactness is checked, not assumed."""
    assert float(want.abs().max()) < EXACT
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.cpu().double(), want)


@functools.lru_cache(maxsize=None)
def nt_case(m, n, k):
    a, bt, bias = ints((m, k), m + n + k), ints((n, k), m + n + k + 1), ints((n,), m + n + k + 2)
    assert 64 * k < EXACT                                      # every partial sum of every order
    return a.to(DEV), bt.to(DEV), bias.to(DEV), a.double() @ bt.double().t(), bias.double()


@functools.lru_cache(maxsize=None)
def tn_case(m, n, k):
    g, a = ints((m, n), m + n + k + 3), ints((m, k), m + n + k + 4)
    assert 64 * m < EXACT
    return g.to(DEV), a.to(DEV), g.double().t() @ a.double()


@pytest.mark.parametrize('shape,splits', G.NT, ids=[f'{m}x{n}x{k}-s{s}' for (m, n, k), s in G.NT])
def test_gemm_nt_equals_float64_bit_for_bit(shape, splits):
    assert G.nt_splits(*shape) == splits
    a, bt, _, want, _ = nt_case(*shape)
    got = ops.gemm_nt(a, bt)
    exact(got, want)
    assert torch.equal(got, ops.gemm_nt(a, bt))


@pytest.mark.parametrize('shape', [(32, 64, 8), (32768, 64, 8), (32, 64, 1096), (96, 2688, 1096), (32, 64, 32776)])   # splits 1, 1, 17, 17, 512
def test_gemm_nt_bias_equals_product_plus_bias_exactly(shape):
    a, bt, bias, want, bias64 = nt_case(*shape)
    exact(ops.gemm_nt(a, bt, bias=bias), want + bias64)


@pytest.mark.parametrize('shape,splits', G.TN, ids=[f'{m}x{n}x{k}-s{s}' for (m, n, k), s in G.TN])
def test_gemm_tn_equals_float64_bit_for_bit(shape, splits):
    assert G.tn_splits(*shape) == splits
    g, a, want = tn_case(*shape)
    got = ops.gemm_tn(g, a)
    exact(got, want)
    assert torch.equal(got, ops.gemm_tn(g, a))


def col_blocks(x, batch):
    """(M, batch * C) -> its column blocks as a (batch, M, C) view: strides (C, batch * C, 1), no copy."""
    return x.view(x.shape[0], batch, x.shape[1] // batch).permute(1, 0, 2)


@functools.lru_cache(maxsize=None)
def batched_case(m, n, k, batch):
    """Two pairs of operands, each one wider matrix whose column blocks are the batch: (gw, aw, gw2, aw2) on the device and the float64
    products and column sums of each pair."""
    seed = m + n + k + batch
    wide = [ints((m, batch * c), seed + i) for i, c in enumerate((n, k, n, k))]
    assert 2 * 64 * m < EXACT
    blk = [col_blocks(x.double(), batch) for x in wide]
    prods = [torch.einsum('bmn,bmk->bnk', blk[0], blk[1]), torch.einsum('bmn,bmk->bnk', blk[2], blk[3])]
    sums = [blk[0].sum(1), blk[2].sum(1)]
    return [x.to(DEV) for x in wide], prods, sums


@pytest.mark.parametrize('two_pairs,colsum_of', [(False, 0), (False, 1), (True, 0), (True, 1), (True, 2)])
@pytest.mark.parametrize('shape,splits', G.BATCHED, ids=[f'{m}x{n}x{k}x{b}-s{s}' for (m, n, k, b), s in G.BATCHED])
def test_gemm_tn_batched_equals_float64_bit_for_bit(shape, splits, two_pairs, colsum_of):
    m, n, k, batch = shape
    assert G.batched_splits(m, n, k, batch, colsum_of != 0) == splits
    wide, prods, sums = batched_case(*shape)
    strided = [col_blocks(x, batch) for x in wide]
    dense = [x.contiguous() for x in strided]
    assert not strided[0].is_contiguous() or batch == 1
    want = prods[0] + prods[1] if two_pairs else prods[0]
    results = []
    for g, a, g2, a2 in (strided, dense):
        out = ops.gemm_tn_batched(g, a, g2=g2 if two_pairs else None, a2=a2 if two_pairs else None, colsum_of=colsum_of)
        c, cs = out if colsum_of else (out, None)
        exact(c, want)
        if colsum_of:
            exact(cs, sums[colsum_of - 1])
        results.append((c, cs))
    assert torch.equal(results[0][0], results[1][0])          # operands in place and copied: the same bits
    if colsum_of:
        assert torch.equal(results[0][1], results[1][1])


# ---- poisoned scratch, guarded output -------------------------------------------------------------------------------------------------------
GUARD = 64                                                    # guard rows in front of and behind the output


def poisoned(nbytes):
    return torch.full((max(nbytes, 256) // 4,), NAN_BITS, dtype=torch.int32, device=DEV)


def guarded(shape):
    """A NaN-filled tensor of `shape` inside a larger allocation with GUARD sentinel rows of its last dimension on both sides."""
    cols = shape[-1]
    rows = 1
    for s in shape[:-1]:
        rows *= s
    big = torch.full((GUARD + rows + GUARD, cols), SENTINEL, device=DEV)
    view = big[GUARD:GUARD + rows].view(shape)
    view.fill_(float('nan'))
    return big, view


def guards_hold(big):
    return bool((big[:GUARD] == SENTINEL).all()) and bool((big[-GUARD:] == SENTINEL).all())


def check_scratch(scratch, need):
    """An unsplit call leaves the scratch alone; a split one has written every partial it then read (the result is exact, so no NaN was
    added in) and nothing behind them."""
    bits = scratch.cpu()
    if need == 0:
        assert bool((bits == NAN_BITS).all())
    else:
        assert bool((bits[need // 4:] == NAN_BITS).all())
        assert not bool((bits[:need // 4] == NAN_BITS).any())


@pytest.mark.parametrize('shape', [(32, 64, 8), (160, 64, 4104), (32, 64, 1096)])                  # splits 1, 64, 17
@pytest.mark.parametrize('with_bias', [False, True])
def test_gemm_nt_with_poisoned_scratch_and_guarded_output(shape, with_bias):
    m, n, k = shape
    a, bt, bias, want, bias64 = nt_case(*shape)
    need = 4 * m * n * G.nt_splits(*shape) if G.nt_splits(*shape) > 1 else 0
    scratch = poisoned(need + 1024)
    big, out = guarded((m, n))
    got = ops.gemm_nt(a, bt, bias=bias if with_bias else None, out=out, scratch=scratch)
    assert got.data_ptr() == out.data_ptr()
    exact(out, want + bias64 if with_bias else want)
    assert guards_hold(big)
    check_scratch(scratch, need)
    if need:
        with pytest.raises(ValueError, match='scratch'):
            ops.gemm_nt(a, bt, out=out, scratch=torch.empty(need - 1, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize('shape', [(8, 32, 64), (4104, 160, 64), (1096, 32, 64)])                  # splits 1, 64, 17
def test_gemm_tn_with_poisoned_scratch_and_guarded_output(shape):
    m, n, k = shape
    g, a, want = tn_case(*shape)
    need = 4 * n * k * G.tn_splits(*shape) if G.tn_splits(*shape) > 1 else 0
    scratch = poisoned(need + 1024)
    big, out = guarded((n, k))
    ops.gemm_tn(g, a, out=out, scratch=scratch)
    exact(out, want)
    assert guards_hold(big)
    check_scratch(scratch, need)
    if need:
        with pytest.raises(ValueError, match='scratch'):
            ops.gemm_tn(g, a, out=out, scratch=torch.empty(need - 1, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize('shape', [(64, 64, 128, 4), (136, 64, 64, 2), (1096, 64, 256, 1)])         # splits 1, 2, 17
@pytest.mark.parametrize('two_pairs,colsum_of', [(False, 1), (True, 2), (True, 0)])
def test_gemm_tn_batched_with_poisoned_scratch_and_guarded_output(shape, two_pairs, colsum_of):
    m, n, k, batch = shape
    wide, prods, sums = batched_case(*shape)
    g, a, g2, a2 = (col_blocks(x, batch) for x in wide)
    splits = G.batched_splits(m, n, k, batch, colsum_of != 0)
    need = 4 * batch * (n * k + (n if colsum_of else 0)) * splits if splits > 1 else 0
    scratch = poisoned(need + 1024)
    big, out = guarded((batch, n, k))
    big_s, cs = guarded((batch, n))
    ops.gemm_tn_batched(g, a, g2=g2 if two_pairs else None, a2=a2 if two_pairs else None, colsum_of=colsum_of,
                        out=(out, cs) if colsum_of else out, scratch=scratch)
    exact(out, prods[0] + prods[1] if two_pairs else prods[0])
    if colsum_of:
        exact(cs, sums[colsum_of - 1])
    else:
        assert bool(torch.isnan(cs).all())                    # no column sums asked for: none written
    assert guards_hold(big) and guards_hold(big_s)
    check_scratch(scratch, need)
    if need:
        with pytest.raises(ValueError, match='scratch'):
            ops.gemm_tn_batched(g, a, colsum_of=colsum_of, out=(out, cs) if colsum_of else out,
                                scratch=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
