"""ops.act_gate (csrc/act_gate.hip) on the GPU: d = g * mul * act'(y) from `out` and `mul` alone, bit for bit against the
same formula written with torch's elementwise ops (each one rounding, nothing contracted), on the shapes of tests/fusion_bwd_ref.py -
one quad, two small images, more than one block per image with odd sizes, three images - with mul absent, positive, of mixed sign and
with zeros, and y == 0 entries; against float64 at the project's bar; NaN-filled guard rows around the output; in place; the amax word;
the NaN and zero rules; two runs."""
import numpy as np
import pytest
import torch

from tests import conv3x3_ref as R
from tests import fusion_bwd_ref as G
from thesis_clip_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = [(shape, kind, act) for shape in G.GATE_SHAPES for kind in G.MUL_KINDS for act in G.ACTS]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def case(shape, kind, act):
    g, y, mul = G.gate_inputs(shape, kind)
    return g, y, mul, dev(g), dev(G.forward32(y, mul, act)), dev(mul)


def torch_formula(g, out, mul, act):
    m = torch.ones_like(out) if mul is None else mul[:, None, None, :].expand_as(out)
    positive = ((out > 0) & (m > 0)) | ((out < 0) & (m < 0))
    straight = g * m
    if act is None:
        d = straight
    elif act == 'relu':
        d = torch.where(positive, straight, torch.zeros_like(g))
    else:
        d = torch.where(positive, straight, g * (out + m))
    return torch.where(m == 0, torch.zeros_like(g), d)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('shape,kind,act', CASES, ids=str)
def test_bits_guards_in_place_amax_and_two_runs(shape, kind, act):
    g_np, y_np, mul_np, g, out, mul = case(shape, kind, act)
    n, h, w, c = shape
    want = torch_formula(g, out, mul, act)
    guard = 2 * c
    buf = torch.full((g.numel() + 2 * guard,), float('nan'), device=DEV)
    d = buf[guard:guard + g.numel()].view(shape)
    word = torch.full((1,), 7.0, device=DEV)
    assert ops.act_gate(g, out, mul, act, out_d=d, amax_out=word) is d
    torch.cuda.synchronize()
    assert same_bits(d, want)
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + g.numel():]).all()
    assert float(word) == float(want.abs().max())
    if kind == 'with_zero':
        assert not d[..., ::3].contiguous().view(torch.int32).any()               # exact +0 under mul == 0
    word2 = torch.full((1,), -1.0, device=DEV)
    assert same_bits(ops.act_gate(g, out, mul, act, amax_out=word2), d) and same_bits(word, word2)      # again, into fresh memory
    g2 = g.clone()
    assert ops.act_gate(g2, out, mul, act, out_d=g2) is g2 and same_bits(g2, want)                          # in place: d = g
    ref = G.gate_ref(g_np, y_np, mul_np, act)
    if ref.any():
        err, yard = R.errors(d.cpu().numpy(), ref), G.gate_e32(shape, kind, act)
        print(f'{shape} {kind} {act}: e64 = {err[0]:.3g}, {err[1]:.3g}; e32 = {yard[0]:.3g}, {yard[1]:.3g}')
        assert G.within_bar(err, yard), (err, yard)


def test_identity_nan_and_zero_rules():
    shape = (2, 3, 5, 32)
    g_np, y_np, mul_np, g, out, mul = case(shape, 'mixed', 'elu')
    assert same_bits(ops.act_gate(g, out, mul, None), torch_formula(g, out, mul, None))
    assert same_bits(ops.act_gate(g, out, None, 'identity'), g)
    # a NaN in g where the gate is open: a NaN in d and in the amax word; under mul == 0 it is an exact zero
    word = torch.zeros(1, device=DEV)
    bad = g.clone()
    bad[1, 2, 4, 7] = float('nan')
    for act in G.ACTS:
        ones = torch.ones_like(out)
        d = ops.act_gate(bad, ones, None, act, amax_out=word)
        assert torch.isnan(d[1, 2, 4, 7]) and int(torch.isnan(d).sum()) == 1 and torch.isnan(word).all()
        zero = torch.zeros_like(mul)
        d = ops.act_gate(bad, out, zero, act, amax_out=word)
        assert not d.view(torch.int32).any() and float(word) == 0.0
    # out == 0 everywhere (a dead relu map): zeros; the elu branch gives g * mul there (elu'(0) == 1)
    dead = torch.zeros_like(out)
    assert not ops.act_gate(g, dead, mul, 'relu', amax_out=word).view(torch.int32).any() and float(word) == 0.0
    assert same_bits(ops.act_gate(g, dead, mul, 'elu'), g * mul[:, None, None, :])


def test_argument_errors_name_the_argument():
    g, out = torch.zeros(2, 3, 5, 32, device=DEV), torch.zeros(2, 3, 5, 32, device=DEV)
    with pytest.raises(ValueError, match='out: must live on a HIP device'):
        ops.act_gate(g, out.cpu(), None, 'relu')
    with pytest.raises(ValueError, match='g: must be contiguous'):
        ops.act_gate(torch.zeros(2, 3, 32, 5, device=DEV).permute(0, 1, 3, 2), out, None, 'relu')
    with pytest.raises(ValueError, match='mul: dtype'):
        ops.act_gate(g, out, torch.zeros(2, 32, device=DEV, dtype=torch.float64), 'relu')
    with pytest.raises(ValueError, match='amax_out: shape'):
        ops.act_gate(g, out, None, 'relu', amax_out=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError, match='out_d: must be 16-byte aligned'):
        ops.act_gate(g, out, None, 'relu', out_d=torch.zeros(g.numel() + 1, device=DEV)[1:].view(g.shape))
