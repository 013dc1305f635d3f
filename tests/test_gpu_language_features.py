"""The language-conditioned feature maps on the GPU at a tiny configuration (32 x 32 images, reduced widths): the fused tail inside
CombineCLIPVisualV4 and CombineCLIPVisualV0 against their torch tails, the 'auto' switch under gradients, an instruction that reaches
LanguageNeRF, and one training step on encoded batches.  The kernel alone is tests/test_gpu_feature_tail.py."""
import numpy as np
import pytest
import torch

from tests import feature_fusion_ref as R
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import train_language as T
from thesis_clip_nerf_amd.grasp_optimizer import DEFAULT_WORKSPACE_BOUNDS as BOUNDS
from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF, kl_divergence
from thesis_clip_nerf_amd.synthetic import glorot_net

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TINY_VISUAL = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(4, 8, 16, 32))
TINY_FUSION = dict(clip_channels=(16, 32, 32, 64), text_dim=64, widths=(64, 32, 32), up3_filters=16)


def tiny_producer(**kw):
    torch.manual_seed(0)
    return E.LanguageFeatureProducer((32, 32), n_features=32, clip_pyramid=E.SyntheticCLIPPyramid((16, 32, 32, 64), (8, 4, 2, 1), 64),
                                     clip_text=E.SyntheticCLIPText(embed_dim=64), combine_kw=TINY_FUSION, **TINY_VISUAL, **kw).to(DEV)


def fusion_inputs(n, device, dtype):
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g).to(device=device, dtype=dtype)
    clip = (r(n, 64), r(n, 16, 8, 8), r(n, 32, 4, 4), r(n, 32, 2, 2), r(n, 64, 1, 1))
    return clip, r(n, 32, 16, 16), r(n, 64)


def check_fused_against_torch(run, module):
    """run(module, device, dtype) -> NCHW / NHWC output.  The fused run and the float32 torch run on the GPU, both against the float64
    run of the module on the CPU: the fused error may be 8 x the torch run's (relative L2 and worst element), as for the kernel alone."""
    module.fused_tail = False
    ref = run(module.double().cpu(), 'cpu', torch.float64).numpy()
    module.float().to(DEV)
    with torch.no_grad():
        plain = run(module, DEV, torch.float32).cpu().numpy()
        module.fused_tail = True
        fused = run(module, DEV, torch.float32).cpu().numpy()
    assert fused.shape == ref.shape
    e_plain, e_fused = (R.rel_l2(plain, ref), R.worst(plain, ref)), (R.rel_l2(fused, ref), R.worst(fused, ref))
    print(f'torch tail {e_plain}, fused tail {e_fused}')
    assert 0 < e_plain[0] < 1e-4                                                    # float32 rounding through the whole module
    assert e_fused[0] <= R.TAIL_BAR * e_plain[0] and e_fused[1] <= R.TAIL_BAR * e_plain[1], (e_fused, e_plain)


def test_combine_clip_visual_v4_fused_tail_against_torch():
    torch.manual_seed(1)
    mod = E.CombineCLIPVisualV4(use_dense=True, activation='elu', half_size=(16, 16), visual_channels=32, **TINY_FUSION).requires_grad_(False)

    def run(m, device, dtype):
        clip, visual, text = fusion_inputs(2, device, dtype)
        with torch.no_grad():
            out = m(clip, visual, text)
        assert out.shape == (2, 256, 32, 32)
        return out.permute(0, 2, 3, 1).contiguous()
    check_fused_against_torch(run, mod)
    clip, visual, text = fusion_inputs(2, DEV, torch.float32)
    out16 = mod(clip, visual, text, out_dtype=torch.bfloat16)                       # the kernel writes bf16 itself
    assert out16.dtype == torch.bfloat16 and torch.equal(out16, mod(clip, visual, text).to(torch.bfloat16))


def test_combine_clip_visual_v0_fused_tail_against_torch():
    """The image-only producer's fusion (act = identity, 256 + 256 channels) with fused_tail=True against its torch tail."""
    torch.manual_seed(2)
    mod = E.CombineCLIPVisualV0((16, 16), 256, 256, 256).requires_grad_(False)
    assert mod.fused_tail is False                                                  # the default stays torch

    def run(m, device, dtype):
        g = torch.Generator().manual_seed(3)
        clip = torch.randn(2, 256, 7, 7, generator=g).to(device=device, dtype=dtype)
        visual = torch.randn(2, 256, 16, 16, generator=g).to(device=device, dtype=dtype)
        with torch.no_grad():
            out = m(clip, visual)
        assert out.shape == (2, 256, 32, 32)
        return out.permute(0, 2, 3, 1).contiguous()
    check_fused_against_torch(run, mod)


def test_auto_takes_the_torch_path_under_gradients(monkeypatch):
    from thesis_clip_nerf_amd import ops
    calls = []
    fuse = ops.fuse_upsample2x
    monkeypatch.setattr(ops, 'fuse_upsample2x', lambda *a, **kw: calls.append(1) or fuse(*a, **kw))
    torch.manual_seed(4)
    mod = E.CombineCLIPVisualV4(use_dense=True, activation='elu', half_size=(16, 16), visual_channels=32, **TINY_FUSION).to(DEV)
    assert mod.fused_tail == 'auto'
    clip, visual, text = fusion_inputs(1, DEV, torch.float32)
    out = mod(clip, visual, text)
    assert out.requires_grad and not calls
    out.square().mean().backward()
    g = mod.conv_fusion_3.conv.weight.grad
    assert g is not None and float(g.abs().sum()) > 0
    with torch.no_grad():
        fused = mod(clip, visual, text)                                              # nothing needs a gradient: the fused pass
    assert not fused.requires_grad and len(calls) == 1
    assert R.rel_l2(fused.cpu().numpy(), out.detach().cpu().numpy()) < 1e-5


@pytest.fixture(scope='module')
def encoded():
    ds = T.SyntheticLanguageDataset(n_scenes=4, n_perspectives=5, height=32, width=32, seed=0)
    return T.EncodedLanguageDataset(ds, tiny_producer(), DEV)


def make_model(seed, batch=2, paf=2, n_future=6):
    torch.manual_seed(seed)
    model = LanguageNeRF(glorot_net(np.random.default_rng(seed), bias_scale=0.05), n_points_train=paf * n_future, n_views=1,
                         batch_size=batch, rotation_representation='6d', softmax_before_loss=True, device=DEV)
    model.compile(loss=kl_divergence, learning_rate=1e-4)
    return model


def test_the_instruction_reaches_the_model(encoded):
    first = encoded.feature_map(1, 0, instruction='pick up the red block')
    second = encoded.feature_map(1, 0, instruction='pick up the blue mug')
    assert isinstance(first, torch.Tensor) and first.device == torch.device(DEV) and first.shape == (32, 32, 256) and first.is_contiguous()
    assert R.rel_l2(second.cpu().numpy(), first.cpu().numpy()) > 1e-3
    assert torch.equal(encoded.feature_map(1, 0, instruction='pick up the red block'), first)           # the same instruction: the same bits
    assert torch.equal(encoded.feature_map(1, 0), encoded.feature_map(1, 0, instruction=encoded.instruction(1)))
    model = make_model(3)
    input_data, _, _, grasp = T.get_inputs(encoded, 1, 3, device=DEV, with_tokens=True)
    assert input_data[3].dtype == torch.int32 and input_data[3].shape == (1, 77)
    inputs = [None] * 4 + [x[:, :1].contiguous() for x in input_data[:3]]             # one view
    rng = np.random.default_rng(0)
    transforms = np.tile(grasp, (1, 8, 1, 1)).astype(np.float32)
    transforms[0, :, :3, 3] += 0.02 * rng.standard_normal((8, 3)).astype(np.float32)
    maps = lambda text: torch.stack([encoded.feature_map(1, p, instruction=text) for p in range(1)])[None]
    out_a = model.infer(inputs, transforms, 8, maps('pick up the red block'))
    out_b = model.infer(inputs, transforms, 8, maps('pick up the blue mug'))
    assert torch.isfinite(out_a).all() and not torch.equal(out_a, out_b)
    assert torch.equal(model.infer(inputs, transforms, 8, maps('pick up the red block')), out_a)


def test_train_step_on_encoded_batches(encoded):
    gen = T.LanguageDataGenerator(encoded, BOUNDS, n_views=1, batch_size=2, shuffle=False, pose_augmentation_factor=2, n_future_poses=6,
                                  rotation_representation='6d', device=DEV, with_tokens=True)
    np.random.seed(0)
    (inputs, features), labels = gen[0]
    assert inputs[7].dtype == torch.int32 and inputs[7].shape == (2, 77) and inputs[7].device == torch.device(DEV)
    assert torch.equal(inputs[7].cpu(), torch.from_numpy(np.stack([encoded.tokens(0), encoded.tokens(1)])))
    assert features.shape == (2, 1, 32, 32, 256) and features.device == torch.device(DEV) and features.dtype == torch.float32
    out = make_model(5).train_step((inputs, labels), features)
    assert all(bool(torch.isfinite(out[k]).all()) for k in ('landscape_loss', 'grad_loss_t', 'grad_loss_r'))
