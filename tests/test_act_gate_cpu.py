"""The backward through a frozen 3x3 convolution of the language fusion, without a GPU: the host build of
csrc/mvnerf_act_gate.h (tests/cpu_act_gate) bit for bit against the NumPy restatement of tests/fusion_bwd_ref.py; the restatement against
float64 autograd of act(y) * mul at the project's bar e64 <= 8 e32, e32 being torch's float32 autograd of the same case, with mul absent,
positive, of mixed sign and with zeros, and y == 0 entries; planted defects against the same assertion; the float64 reference of the
two-source data gradients against torch in float64; the argument checks of the entry point and of ops.act_gate; the new switches, the
producer and the checkpoint rules on CPU tensors.  The kernel itself is tests/test_gpu_act_gate.py, the modules tests/test_gpu_fusion_backward.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import conv3x3_ref as R
from tests import fusion_bwd_ref as G
from thesis_clip_nerf_amd import _lib
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
TINY_VIT = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(4, 8, 16, 32))
TINY_FUSION = dict(clip_channels=(32, 32, 32, 32), text_dim=64, widths=(64, 64, 64), up3_filters=64)
CASES = [(shape, kind, act) for shape in G.GATE_SHAPES for kind in G.MUL_KINDS for act in G.ACTS]


@pytest.fixture(scope='module')
def cpu():
    d = os.path.join(HERE, 'cpu_act_gate')
    subprocess.run(['make', '-C', d], check=True, capture_output=True)
    lib = ctypes.CDLL(os.path.join(d, 'libmvnerf_act_gate_cpu.so'))
    lib.act_gate_cpu.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
    lib.act_gate_cpu.restype = None
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_gate(cpu, g, out, mul, act, in_place=False):
    g, out = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(out, np.float32)
    mul = None if mul is None else np.ascontiguousarray(mul, np.float32)
    n, h, w, c = g.shape
    d = g.copy() if in_place else np.full_like(g, np.nan)
    cpu.act_gate_cpu(ptr(d if in_place else g), ptr(out), ptr(mul), G.ACT_CODES[act], n, h * w, c, ptr(d))
    return d


def same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32))


@pytest.mark.parametrize('shape,kind,act', CASES, ids=str)
def test_host_build_equals_the_restatement_bit_for_bit(cpu, shape, kind, act):
    g, y, mul = G.gate_inputs(shape, kind)
    out = G.forward32(y, mul, act)
    want = G.gate_np(g, out, mul, act)
    assert same_bits(host_gate(cpu, g, out, mul, act), want)
    assert same_bits(host_gate(cpu, g, out, mul, act, in_place=True), want)
    if kind == 'with_zero':
        assert not want[:, :, :, ::3].any() and not np.signbit(want[:, :, :, ::3]).any()


def test_host_build_identity_and_edge_values(cpu):
    g, y, mul = G.gate_inputs((2, 3, 5, 32), 'mixed')
    assert same_bits(host_gate(cpu, g, y, mul, None), (g * mul[:, None, None, :]).astype(np.float32))
    # factors whose product out * mul underflows: the sign test still sees act(y) > 0 (relu passes, elu takes the straight branch)
    tiny = np.full((1, 1, 1, 4), 1e-30, np.float32)
    out = tiny * np.array([1, -1, 1, -1], np.float32)
    mul = np.array([[1e-30, -1e-30, -1e-30, 1e-30]], np.float32)
    g1 = np.ones((1, 1, 1, 4), np.float32)
    assert float(out[0, 0, 0, 0]) * float(mul[0, 0]) < 1e-45
    for act in G.ACTS:
        d = host_gate(cpu, g1, out, mul, act)[0, 0, 0]
        assert d[0] == mul[0, 0] and d[1] == mul[0, 1]
        if act == 'relu':
            assert d[2] == 0 and d[3] == 0
        assert same_bits(d, G.gate_np(g1, out, mul, act)[0, 0, 0])
    # mul == 0: an exact +0 whatever g holds
    wild = np.array([np.inf, -np.inf, np.nan, -1.0], np.float32).reshape(1, 1, 1, 4)
    for act in (None, 'relu', 'elu'):
        d = host_gate(cpu, wild, np.zeros((1, 1, 1, 4), np.float32), np.zeros((1, 4), np.float32), act)
        assert same_bits(d, np.zeros_like(d))
    # a NaN in g passes where the gate is open
    d = host_gate(cpu, wild, np.ones((1, 1, 1, 4), np.float32), None, 'relu')
    assert np.isnan(d[0, 0, 0, 2]) and d[0, 0, 0, 3] == -1.0


@pytest.mark.parametrize('shape,kind,act', CASES, ids=str)
def test_restatement_meets_the_bar_against_float64(shape, kind, act):
    g, y, mul = G.gate_inputs(shape, kind)
    ref = G.gate_ref(g, y, mul, act)
    assert R.worst(G.torch_gate(g, y, mul, act, torch.float64), ref) <= 1e-15
    if not ref.any():
        assert not G.gate_np(g, G.forward32(y, mul, act), mul, act).any()
        return
    err, yard = R.errors(G.gate_np(g, G.forward32(y, mul, act), mul, act), ref), G.gate_e32(shape, kind, act)
    print(f'{shape} {kind} {act}: e64 = {err[0]:.3g}, {err[1]:.3g}; e32 = {yard[0]:.3g}, {yard[1]:.3g}')
    assert G.within_bar(err, yard), (err, yard)


def test_float64_statement_from_out_and_mul_equals_autograd():
    """The formula itself, free of float32 rounding: d from (out, mul) in float64 against autograd from y, to 1e-15."""
    for kind in G.MUL_KINDS:
        for act in G.ACTS:
            g, y, mul = (None if v is None else v.astype(np.float64) for v in G.gate_inputs((2, 19, 35, 64), kind))
            rows = 1.0 if mul is None else mul[:, None, None, :]
            out = R.activation(y, act) * rows
            m = np.broadcast_to(rows, out.shape)
            positive = ((out > 0) & (m > 0)) | ((out < 0) & (m < 0))
            d = np.where(positive, g * m, 0.0 if act == 'relu' else g * (out + m))
            d = np.where(m == 0, 0.0, d)
            assert np.abs(d - G.torch_gate(g, y, mul, act, torch.float64)).max() <= 1e-15


@pytest.mark.parametrize('defect', G.DEFECTS)
def test_planted_defects_leave_the_bar(defect):
    shape, kind = (2, 19, 35, 64), 'mixed'
    acts = {'relu_passes_at_zero': ['relu'], 'elu_branch_from_out': ['elu'], 'mul_forgotten': ['elu']}.get(defect, G.ACTS)
    for act in acts:
        g, y, mul = G.gate_inputs(shape, kind)
        out = G.forward32(y, mul, act)
        ref = G.gate_ref(g, y, mul, act)
        yard = G.gate_e32(shape, kind, act)
        assert G.within_bar(R.errors(G.gate_np(g, out, mul, act), ref), yard)
        assert not G.within_bar(R.errors(G.gate_np(g, out, mul, act, defect=defect), ref), yard), (defect, act)


@pytest.mark.parametrize('kind', ['none', 'mixed', 'with_zero'])
@pytest.mark.parametrize('act', G.ACTS)
def test_two_source_reference_against_float64_torch(kind, act):
    for shape in ((2, 3, 5, 64, 32, 64), (1, 5, 4, 64, 0, 64)):
        a, b, wt, mul, g = G.two_source_inputs(shape, kind)
        ref = G.two_source_grads_ref(a, b, wt, mul, act, g)
        got = G.torch_two_source_grads(a, b, wt, mul, act, g, torch.float64)
        assert R.worst(got[0], ref[0]) <= 1e-12
        assert (b is None and ref[1] is None) or R.worst(got[1], ref[1]) <= 1e-12


def test_entry_point_checks_its_arguments_before_any_launch():
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    gate = lambda g=one, out=one, mul=None, act=1, n=1, pixels=8, c=64, d=one, amax=None: lib.mvnerf_act_gate_nhwc(
        g, out, mul, act, n, pixels, c, d, amax, None)
    assert gate(g=None) == -1 and b'(g)' in lib.mvnerf_last_error()
    assert gate(out=None) == -1 and b'(out)' in lib.mvnerf_last_error()
    assert gate(d=None) == -1 and b'(d)' in lib.mvnerf_last_error() and b'mvnerf_act_gate_nhwc' in lib.mvnerf_last_error()
    assert gate(n=0) == -1 and gate(n=65536) == -1 and b'N=65536' in lib.mvnerf_last_error()
    assert gate(pixels=0) == -1 and gate(n=3, pixels=2 ** 30) == -1 and b'pixels_per_image' in lib.mvnerf_last_error()
    assert gate(c=6) == -2 and b'C=6' in lib.mvnerf_last_error() and gate(c=0) == -2
    assert gate(act=3) == -2 and b'act=3' in lib.mvnerf_last_error() and gate(act=-1) == -2
    assert gate(g=odd) == -3 and b'g must' in lib.mvnerf_last_error()
    assert gate(mul=odd) == -3 and b'mul must' in lib.mvnerf_last_error()
    assert gate(d=odd) == -3 and gate(out=odd) == -3
    assert gate(amax=ctypes.c_void_p(18)) == -3 and b'amax_out' in lib.mvnerf_last_error()


def test_ops_act_gate_refuses_bad_arguments_and_host_tensors():
    g, out = torch.zeros(2, 3, 5, 32), torch.zeros(2, 3, 5, 32)
    with pytest.raises(ValueError, match='act'):
        ops.act_gate(g, out, None, 'gelu')
    with pytest.raises(ValueError, match='act'):
        ops.act_gate(g, out, None, 3)
    with pytest.raises(ValueError, match='g: 30 channels'):
        ops.act_gate(torch.zeros(1, 2, 2, 30), torch.zeros(1, 2, 2, 30), None, 'relu')
    with pytest.raises(ValueError, match='g: shape'):
        ops.act_gate(torch.zeros(4, 32), torch.zeros(4, 32), None, 'relu')
    with pytest.raises(ValueError, match='out: shape'):
        ops.act_gate(g, torch.zeros(2, 3, 5, 64), None, 'relu')
    with pytest.raises(ValueError, match='mul: shape'):
        ops.act_gate(g, out, torch.zeros(1, 32), 'relu')
    with pytest.raises(ValueError, match='out_d: shape'):
        ops.act_gate(g, out, None, 'relu', out_d=torch.zeros(2, 3, 5, 16))
    with pytest.raises(ValueError, match='g: must live on a HIP device'):
        ops.act_gate(g, out, torch.zeros(2, 32), 'elu')


def tiny_fusion(**kw):
    return E.CombineCLIPVisualV4(half_size=(16, 24), visual_channels=32, **TINY_FUSION, **kw)


def fusion_inputs(n=2, seed=0):
    gen = torch.Generator().manual_seed(seed)
    sizes = ((8, 12), (4, 6), (2, 3), (1, 2))
    maps = [torch.rand(n, c, *s, generator=gen) for c, s in zip(TINY_FUSION['clip_channels'], sizes)]
    return (torch.zeros(n, 64), *maps), torch.randn(n, 32, 16, 24, generator=gen), torch.randn(n, 64, generator=gen)


def test_switches_on_the_cpu():
    with pytest.raises(ValueError, match='fused_backward'):
        E.DoubleConv(64, 64, fused_backward='yes')
    with pytest.raises(ValueError, match='fused_backward'):
        E.Up((8, 8), 64, 32, 64, fused_backward=1)
    up = E.Up((8, 8), 64, 32, 64)
    assert up.fused_backward is False and up.double_conv.fused_backward is False
    up.fused_backward = True
    assert up.double_conv.fused_backward is True
    torch.manual_seed(5)
    mod = tiny_fusion().requires_grad_(False)
    assert mod.fused_backward is False and not any(u.fused_backward for u in (mod.up_1, mod.up_2, mod.up_3))
    clip, vis, text = fusion_inputs()
    vis.requires_grad_(True)
    plain = mod(clip, vis, text)
    grad, = torch.autograd.grad(plain.square().mean(), vis)
    mod.fused_conv, mod.fused_backward = 'auto', True             # CPU tensors: the torch path, the same bits in both directions
    assert all(u.fused_backward is True and u.fused_conv == 'auto' for u in (mod.up_1, mod.up_2, mod.up_3))
    again = mod(clip, vis, text)
    assert torch.equal(again, plain)
    assert torch.equal(torch.autograd.grad(again.square().mean(), vis)[0], grad)
    assert all(p.grad is None for p in mod.parameters())
    with pytest.raises(ValueError, match='fused_backward'):
        mod.fused_backward = 'auto'


def tiny_producer(**kw):
    pyramid = E.SyntheticCLIPPyramid(TINY_FUSION['clip_channels'], ((8, 8), (4, 4), (2, 2), (1, 1)), TINY_FUSION['text_dim'])
    return E.FeatureProducerV4((32, 32), n_features=32, clip_pyramid=pyramid, combine_kw=TINY_FUSION, **TINY_VIT, **kw)


def test_feature_producer_v4_on_the_cpu():
    torch.manual_seed(1)
    prod = tiny_producer()
    fusion = prod.combine_clip_visual
    assert fusion.activation == 'relu' and fusion.multiply_fusion_1.tile.dense is None and fusion.fused_backward is False
    other = tiny_producer(use_dense=True, activation='elu', fused_conv='auto', fused_backward=True, fused_visual='auto')
    assert other.combine_clip_visual.activation == 'elu' and other.combine_clip_visual.multiply_fusion_1.tile.dense is not None
    assert other.combine_clip_visual.fused_backward is True and other.visual_features.fused_backward is True
    assert other.visual_features.fused_conv == 'auto' and other.combine_clip_visual.fused_conv == 'auto'
    trainable = {id(p) for p in prod.trainable_parameters()}
    assert trainable == {id(p) for m in (prod.visual_features.vision_transformer, prod.visual_features.conv_features) for p in m.parameters()}
    assert not any(p.requires_grad for p in fusion.parameters()) and all(p.requires_grad for p in prod.trainable_parameters())
    images = torch.rand(2, 32, 32, 3)
    out = prod(images)
    assert out.shape == (2, 32, 32, 256) and out.is_contiguous() and out.requires_grad
    assert torch.equal(out, prod(images, text_embedding=torch.ones(1, 64)))             # None means all ones
    assert not torch.equal(out, prod(images, text_embedding=torch.full((2, 64), 0.5)))
    out.square().mean().backward()
    assert all(p.grad is None for p in fusion.parameters())
    assert any(p.grad is not None and p.grad.abs().sum() > 0 for p in prod.trainable_parameters())
    with pytest.raises(ValueError, match='multiples of 16'):
        E.FeatureProducerV4((24, 32))


class _Renderer:
    """MVVNeRFRenderer's checkpoint methods on host tensors (its constructor needs a GPU)."""
    from thesis_clip_nerf_amd.model import MVVNeRFRenderer as _M
    store, load, _split, _encoder_modules = _M.store, _M.load, _M._split, _M._encoder_modules

    def __init__(self, encoder, seed):
        gen = torch.Generator().manual_seed(seed)
        self.feature_encoder = encoder
        self.coarse_net, self.fine_net = torch.randn(_lib.NET_PARAMS, generator=gen), torch.randn(_lib.NET_PARAMS, generator=gen)

    def set_weights(self, coarse_net=None, fine_net=None):
        self.coarse_net, self.fine_net = coarse_net.clone(), fine_net.clone()


def _state(module):
    return {k: v.clone() for k, v in module.state_dict().items()}


def _same_state(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_checkpoint_rules(tmp_path):
    torch.manual_seed(2)
    src, dst = _Renderer(tiny_producer(), 1), _Renderer(tiny_producer(), 2)
    path = str(tmp_path / 'model_final')
    src.store(path)                                                    # the default: the four MLP files, as before
    assert sorted(os.listdir(tmp_path)) == sorted(f'model_final_{n}.pt' for n in ('coarse_embedding', 'coarse_readout', 'fine_embedding',
                                                                                   'fine_readout'))
    before = (dst.coarse_net.clone(), dst.fine_net.clone(), _state(dst.feature_encoder))
    assert dst.load(path, encoders=True) is False                      # two of the six are missing: nothing changes
    assert torch.equal(dst.coarse_net, before[0]) and torch.equal(dst.fine_net, before[1])
    assert _same_state(_state(dst.feature_encoder), before[2])
    assert dst.load(path) is True and torch.equal(dst.coarse_net, src.coarse_net) and torch.equal(dst.fine_net, src.fine_net)
    assert _same_state(_state(dst.feature_encoder), before[2])         # the default load leaves the encoders alone
    src.store(path, encoders=True)
    assert len(os.listdir(tmp_path)) == 6
    for name in ('visual_features', 'combine_clip_visual'):
        saved = torch.load(f'{path}_{name}.pt', weights_only=True)
        assert all(v.device.type == 'cpu' for v in saved.values()) and _same_state(saved, _state(getattr(src.feature_encoder, name)))
    dst = _Renderer(tiny_producer(), 3)
    assert dst.load(path, encoders=True) is True
    assert torch.equal(dst.coarse_net, src.coarse_net) and _same_state(_state(dst.feature_encoder), _state(src.feature_encoder))
    os.remove(f'{path}_visual_features.pt')
    fresh = _Renderer(tiny_producer(), 4)
    before = (fresh.coarse_net.clone(), _state(fresh.feature_encoder))
    assert fresh.load(path, encoders=True) is False
    assert torch.equal(fresh.coarse_net, before[0]) and _same_state(_state(fresh.feature_encoder), before[1])
    with pytest.raises(ValueError, match='visual_features'):
        _Renderer(None, 5).store(path, encoders=True)


def test_load_backbone_takes_the_encoder_files(tmp_path):
    from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF

    class Model:
        load_backbone = LanguageNeRF.load_backbone

        def __init__(self):
            self.trunk_net = torch.zeros(_lib.NET_PARAMS)

    torch.manual_seed(6)
    src = _Renderer(tiny_producer(), 1)
    path = str(tmp_path / 'model_final')
    src.store(path, encoders=True)
    pyramid = E.SyntheticCLIPPyramid(TINY_FUSION['clip_channels'], ((8, 8), (4, 4), (2, 2), (1, 1)), TINY_FUSION['text_dim'])
    make = lambda **kw: E.LanguageFeatureProducer((32, 32), n_features=32, clip_pyramid=pyramid, clip_text=E.SyntheticCLIPText(embed_dim=64),
                                                  combine_kw=dict(TINY_FUSION, **kw), **TINY_VIT)
    producer, model = make(use_dense=False, activation='relu'), Model()
    assert model.load_backbone(path, verbose=False, producer=producer) is True
    assert torch.equal(model.trunk_net, src.fine_net)
    for name in ('visual_features', 'combine_clip_visual'):
        assert _same_state(_state(getattr(producer, name)), _state(getattr(src.feature_encoder, name)))
    assert not any(p.requires_grad for p in producer.parameters())
    # the same renderer's maps: FeatureProducerV4 with the ones embedding == the language producer with the ones embedding
    # (both in inference mode: the language producer always is, and the ViT's first norm reads its moving statistics there)
    images = torch.rand(1, 32, 32, 3)
    with torch.no_grad():
        assert torch.equal(src.feature_encoder.eval()(images),producer(images, text_embedding=torch.ones(1, 64)))
    # a producer whose fusion has the Dense layers: the first key the file lacks is named, nothing is written
    dense, model = make(), Model()
    before = _state(dense)
    with pytest.raises(ValueError, match='multiply_fusion_1.tile.dense.weight'):
        model.load_backbone(path, verbose=False, producer=dense)
    assert _same_state(_state(dense), before) and not model.trunk_net.any()
    os.remove(f'{path}_combine_clip_visual.pt')
    producer, model = make(use_dense=False, activation='relu'), Model()
    before = _state(producer)
    assert model.load_backbone(path, verbose=False, producer=producer) is False
    assert _same_state(_state(producer), before) and not model.trunk_net.any()
    assert model.load_backbone(path, verbose=False) is True            # without a producer: the trunk alone, as before
