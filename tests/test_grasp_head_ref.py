"""tests/grasp_head_ref.py checked on the CPU: its closed forms equal float64 autograd (double backward included), each mutant of them is
seen by the comparison the GPU test makes, and the seeds the GPU test uses leave next to no pre-activation near the jump of elu''."""
import functools

import pytest
import torch

from tests import grasp_head_ref as R

# the sizes of tests/test_gpu_grasp_head_grade.py: one lane; a second wave / a second workgroup with one valid lane; whole tiles; and the
# _HeadFn case (a multiple of 8 with a ragged last tile)
SIZES = (1, 33, 129, 160, 136)
CAP1, CAP2 = 1e-5, 1e-4                                       # the caps the GPU test puts on the first- and second-pass buffers
WEIGHT_SEED, NEAR, seed_of = R.WEIGHT_SEED, R.NEAR, R.seed_of


@functools.lru_cache(maxsize=None)
def case(n):
    acts, g_y, t = (x.double() for x in R.inputs(n, seed_of(n)))
    w = R.to(R.weights(WEIGHT_SEED), torch.float64)
    pos_c, pos_y = R.own_masks(acts, w)
    return acts, g_y, t, w, pos_c, pos_y


@pytest.mark.parametrize('n', SIZES)
def test_closed_forms_equal_float64_autograd(n):
    acts, g_y, t, w, pos_c, pos_y = case(n)
    fb = R.first_buffers(acts, w, g_y, pos_c, pos_y)
    sb = R.second_buffers(acts, w, g_y, t, pos_c, pos_y)
    ab = R.autograd_buffers(acts, w, g_y, t)
    for name in R.FIRST + R.SECOND:
        got = fb[name] if name in fb else sb[name]
        assert got.shape == ab[name].shape
        for label, blk in R.blocks_of(name, got):
            want = dict(R.blocks_of(name, ab[name]))[label]
            assert R.rel(blk, want) < 1e-12, (label, R.rel(blk, want))
    y, first, second = R.autograd_reference(acts, w, g_y, t)
    assert R.rel(fb['y'], y) < 1e-12
    for name, got, want in zip(('d acts', 'd w4', 'd b4', 'd wc', 'd bc'), R.first_grads(fb, acts), first):
        assert got.shape == want.shape and R.rel(got, want) < 1e-12, (name, R.rel(got, want))
    for name, got, want in zip(('dd w4', 'dd b4', 'dd wc', 'dd bc', 'dd g_y'), R.second_grads(fb, sb, acts, t), second):
        assert got.shape == want.shape and R.rel(got, want) < 1e-12, (name, R.rel(got, want))


@pytest.mark.parametrize('n', SIZES)
def test_both_branches_of_every_decision_are_exercised(n):
    acts, _, _, _, pos_c, pos_y = case(n)
    for k in range(4):
        blk = pos_c[:, 64 * k:64 * k + 64]
        assert blk.any() and not blk.all()
    assert pos_y.any() and not pos_y.all()


@pytest.mark.parametrize('mutant', R.MUTANTS)
@pytest.mark.parametrize('n', SIZES[:4])
def test_every_mutant_moves_a_buffer_past_its_cap(n, mutant):
    """The GPU test's figures (relative L2 and worst row per block) of the mutated closed forms against the right ones: at least one exceeds
    the cap its buffer carries there, so no bar of that test is out of a mutant's reach."""
    acts, g_y, t, w, pos_c, pos_y = case(n)
    good = {**R.first_buffers(acts, w, g_y, pos_c, pos_y), **R.second_buffers(acts, w, g_y, t, pos_c, pos_y)}
    bad = {**R.first_buffers(acts, w, g_y, pos_c, pos_y, mutant=mutant), **R.second_buffers(acts, w, g_y, t, pos_c, pos_y, mutant=mutant)}
    seen = []
    for name in R.FIRST + R.SECOND:
        cap = CAP1 if name in R.FIRST else CAP2
        for (label, b), (_, g) in zip(R.blocks_of(name, bad[name]), R.blocks_of(name, good[name])):
            if R.rel(b, g) > cap and R.worst_row(b, g) > cap:
                seen.append(label)
    assert seen, mutant
    first_wrong = {'p_drop_first': 'p', 'p_drop_second': 'p', 'm_e1_for_e2': 'm', 'r_drop_e1': 'r', 'swap_wc_blocks': 'q', 'gv_drop_e1': 'g_v'}[mutant]
    assert any(label.startswith(first_wrong) for label in seen), (mutant, seen)
    if mutant == 'swap_wc_blocks':                            # blocks 0 and 3 of q stay right: only a per-block comparison pins the wrong ones
        assert not any(label in ('q[:, 0:64]', 'q[:, 192:256]') for label in seen)
        assert 'q[:, 64:128]' in seen and 'q[:, 128:192]' in seen


def test_a_wrong_p_block_hides_in_the_whole_tensor_weight_gradient_bars():
    """What the per-buffer test is for: one wrong entry per row of p_k stays below the 1e-4 whole-tensor bar on dd w4, and far above the cap on
    its own block."""
    acts, g_y, t, w, pos_c, pos_y = case(160)
    fb = R.first_buffers(acts, w, g_y, pos_c, pos_y)
    sb = R.second_buffers(acts, w, g_y, t, pos_c, pos_y)
    wrong = dict(sb, p=sb['p'].clone())
    wrong['p'][:, 70] *= 1.0 + 2e-3
    assert R.rel(R.second_grads(fb, wrong, acts, t)[0], R.second_grads(fb, sb, acts, t)[0]) < CAP2
    assert R.rel(wrong['p'][:, 64:128], sb['p'][:, 64:128]) > CAP2


@pytest.mark.parametrize('n', SIZES)
def test_few_pre_activations_lie_near_the_jump_of_the_second_derivative(n):
    acts, _, _, w, _, _ = case(n)
    count, total = R.near_zero(acts, w, NEAR)
    assert total == n * 320
    print(f'N={n} seed={seed_of(n)}: {count} of {total} pre-activations below {NEAR} in magnitude')
    assert count <= 1e-3 * total
    if n == 136:
        assert count == 0                                     # the _HeadFn test compares with float64 autograd on its own decisions
