"""The fill protocol of tests/step_chains.py on CPU tensors: toy "steps" written in torch, one correct and four with a planted defect of
the kind the protocol is for.  Each planted toy must fail the protocol with the assertion that names its cause; the correct toy passes.
No GPU: the helpers are device-agnostic, and tests/test_gpu_step_chains.py applies the same functions to the C entry points."""
import pytest
import torch

from tests import step_chains as C

N, K = 6, 5
WS_FLOATS = N + 8                                         # the accumulator, then room nobody writes


def inputs():
    g = torch.Generator().manual_seed(3)
    return torch.randn(N, K, generator=g), torch.randn(K, generator=g)


def toy(defect=None):
    """out[i] = (sum_k x[i, k] w[k], twice that), the sum formed in a workspace accumulator as a multi-launch step would."""
    x, w = inputs()

    def step(fill):
        ws = fill(4 * WS_FLOATS, name='workspace')
        out = fill((N, 2), name='out')
        acc = ws.view(torch.float32)[:N]
        if defect != 'adds into an un-zeroed scratch':
            acc.zero_()
        for k in range(K):
            acc += x[:, k] * w[k]
        rows = N - 1 if defect == 'leaves an output row unwritten' else N
        out[:rows, 0] = acc[:rows]
        out[:rows, 1] = 2.0 * acc[:rows]
        if defect == 'reads a scratch element it never wrote':
            out[3, 1] = acc[3] * ws.view(torch.float32)[N + 5]
        if defect == 'writes one element past its workspace':
            torch.as_strided(ws.view(torch.float32), (WS_FLOATS + 1,), (1,))[WS_FLOATS] = 0.5
        return dict(out=out)
    return step


def protocol(step):
    want = toy()(C.Fill(C.NAN_WORD, 'cpu'))                # the "chain": the correct toy on NaN-filled buffers of its own
    C.check_protocol(C.run_fills(step, 'cpu'), want)


def test_filled_buffers_and_their_guards():
    for word in C.FILL_WORDS:
        ws, whole = C.filled(40, word)
        assert ws.dtype == torch.uint8 and ws.numel() == 40 and whole.numel() == (40 + C.TAIL_BYTES) // 4
        out, whole_o = C.filled((3, 5), word)
        assert out.shape == (3, 5) and whole_o.shape == (3 + C.GUARD, 5)
        assert bool((C.bits(out) == word).all()) and bool((C.bits(ws) == word).all())
        ranks, _ = C.filled((4,), word, dtype=torch.int32)
        assert ranks.dtype == torch.int32 and bool((ranks == word).all())
        C.assert_guard(ws, whole, word)
        C.assert_guard(out, whole_o, word)
        whole_o[3, 0] = 7                                  # first guard word
        with pytest.raises(AssertionError, match='wrote past the end'):
            C.assert_guard(out, whole_o, word)
    nan, _ = C.filled((2,), C.NAN_WORD)
    one, _ = C.filled((2,), 0x3F800000)
    assert bool(torch.isnan(nan).all()) and bool((one == 1.0).all())


def test_the_correct_toy_passes():
    protocol(toy())
    x, w = inputs()
    out = toy()(C.Fill(0, 'cpu'))['out']
    assert torch.allclose(out[:, 0], x @ w, atol=1e-6)


def test_a_sum_into_an_unzeroed_scratch_passes_the_zero_fill_alone_and_fails_the_protocol():
    step = toy('adds into an un-zeroed scratch')
    want = toy()(C.Fill(C.NAN_WORD, 'cpu'))['out']
    assert torch.equal(step(C.Fill(0, 'cpu'))['out'], want)                      # what a torch.zeros workspace hides
    with pytest.raises(AssertionError, match='adds into memory it did not zero'):
        protocol(step)


def test_a_read_of_an_unwritten_scratch_element_fails_the_protocol():
    with pytest.raises(AssertionError, match='reads memory it did not write'):
        protocol(toy('reads a scratch element it never wrote'))


def test_a_write_past_the_workspace_fails_the_protocol():
    with pytest.raises(AssertionError, match='wrote past the end of workspace'):
        protocol(toy('writes one element past its workspace'))


def test_an_unwritten_output_row_fails_the_protocol():
    with pytest.raises(AssertionError, match=r'out: 2 of 12 elements hold the fill word under every fill: never written'):
        protocol(toy('leaves an output row unwritten'))


def test_a_step_that_differs_from_its_parts_fails_the_protocol():
    def step(fill):
        out = toy()(fill)
        out['out'][2, 0] = torch.nextafter(out['out'][2, 0], torch.tensor(float('inf')))      # one ulp, the same under every fill
        return out
    with pytest.raises(AssertionError, match='out: 1 of 12 elements differ from the chain of the parts'):
        protocol(step)


def test_order_free_outputs_are_left_to_the_caller_but_must_be_written_and_finite():
    def step(fill):
        out = toy()(fill)
        out['loss'] = fill((1,), name='loss')
        out['loss'][0] = 1.0 + 1e-7 * ((fill.word >> 22) & 3)        # differs between fills: allowed for an order-free output
        return out
    want = toy()(C.Fill(C.NAN_WORD, 'cpu'))
    C.check_protocol(C.run_fills(step, 'cpu'), want, order_free=('loss',))
    with pytest.raises(AssertionError, match='loss: fills'):
        C.check_protocol(C.run_fills(step, 'cpu'), dict(want, loss=torch.ones(1)))
