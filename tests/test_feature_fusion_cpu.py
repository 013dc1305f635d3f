"""The language fusion without a GPU: CombineCLIPVisualV4 (encoders.py; src/lib/mvnerf/layers.py:414-520, 593-660) against the float64
reference written from the Keras semantics (tests/feature_fusion_ref.py) through the Keras-variable importer, its parameter counts, the
producer's shape / layout / dtypes, the reference of the fused tail against torch and against planted mistakes, the argument checks of
mvnerf_fuse_upsample2x, and the tokens in the training data.  The kernel itself is tests/test_gpu_feature_tail.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import feature_fusion_ref as R
from thesis_clip_nerf_amd import _lib
from thesis_clip_nerf_amd import encoders as E
from thesis_clip_nerf_amd import train_language as T
from thesis_clip_nerf_amd.grasp_optimizer import DEFAULT_WORKSPACE_BOUNDS as BOUNDS

TINY_VISUAL = dict(transformer_image_size=(32, 32), patch_size=16, embed_dim=32, num_heads=4, hooks=(1, 2, 3, 4), features=(4, 8, 16, 32))
TINY_FUSION = dict(clip_channels=(16, 32, 32, 64), text_dim=64, widths=(64, 32, 32), up3_filters=16)


def tiny_producer(size=(32, 32), **kw):
    return E.LanguageFeatureProducer(size, n_features=32, clip_pyramid=E.SyntheticCLIPPyramid((16, 32, 32, 64), (8, 4, 2, 1), 64),
                                     clip_text=E.SyntheticCLIPText(embed_dim=64), combine_kw=TINY_FUSION, **TINY_VISUAL, **kw)


def test_reference_sized_fusion_has_the_reference_parameter_counts():
    assert E.count_parameters(E.CombineCLIPVisualV4(use_dense=True)) == 36_814_848
    assert E.count_parameters(E.CombineCLIPVisualV4(use_dense=False)) == 34_979_840
    v3 = E.CombineCLIPVisualV4(use_dense=False, up3_filters=256)                      # CombineCLIPVisualV3: up_3 = Up(256), nothing else
    assert E.count_parameters(v3) == 34_979_840 + 9 * 512 * 128 + 9 * (256 * 256 - 128 * 128) + 128 * 256


def test_tiny_producer_shape_layout_and_dtypes():
    torch.manual_seed(0)
    images = torch.rand(2, 32, 48, 3)
    tokens = E.tokenize(['pick up the red block', 'pick up the blue mug'])
    for dtype in (torch.float32, torch.bfloat16):
        prod = tiny_producer((32, 48), out_dtype=dtype)
        out = prod(images, tokens=tokens)
        assert out.shape == (2, 32, 48, 256) and out.dtype == dtype and out.is_contiguous()          # NHWC, what the gather reads
        assert torch.isfinite(out.float()).all()
        assert not any(p.requires_grad for p in prod.parameters()) and not prod.train().training     # frozen
    one = prod(images, tokens=tokens[:1])                                                             # one instruction for all views
    assert torch.equal(one[0], out[0]) and not torch.equal(one[1], out[1])
    assert torch.equal(prod(images, text_embedding=prod.clip_text(tokens)), out)
    with pytest.raises(ValueError):
        prod(images)
    with pytest.raises(ValueError):
        tiny_producer((40, 48))


@pytest.mark.parametrize('use_dense,activation', [(True, 'elu'), (False, 'relu')])
def test_importer_and_module_against_the_keras_semantics_reference(use_dense, activation):
    """Random Keras-layout variables in `model.weights` order -> load_combine_clip_visual_v4 -> forward in float64 == the stand-alone
    reference to 1e-12: a transposed kernel, a swapped concat, a misplaced activation or a wrong resize all show here."""
    rng = np.random.default_rng(11)
    half, n = (8, 16), 2
    mod = E.CombineCLIPVisualV4(use_dense=use_dense, activation=activation, half_size=half, visual_channels=32, filters=256, fused_tail=False,
                                **TINY_FUSION).double()
    shapes = {'conv': (3, 3, 64, 64), 'multiply_fusion_1.tile.dense': (64, 64), 'up_1.double_conv.conv_1': (3, 3, 96, 32),
              'up_1.double_conv.conv_2': (3, 3, 32, 32), 'multiply_fusion_2.tile.dense': (64, 32), 'conv_fusion_1.conv': (1, 1, 64, 32),
              'up_2.double_conv.conv_1': (3, 3, 64, 32), 'up_2.double_conv.conv_2': (3, 3, 32, 32), 'multiply_fusion_3.tile.dense': (64, 32),
              'conv_fusion_2.conv': (1, 1, 64, 32), 'up_3.double_conv.conv_1': (3, 3, 48, 16), 'up_3.double_conv.conv_2': (3, 3, 16, 16),
              'conv_fusion_3.conv': (1, 1, 48, 256)}
    assert tuple(shapes) == E.COMBINE_CLIP_VISUAL_V4_VARIABLES
    names = [k for k in shapes if use_dense or not k.endswith('.dense')]
    arrays = [(rng.standard_normal(shapes[k]) / np.sqrt(np.prod(shapes[k][:-1]))).astype(np.float32) for k in names]
    E.load_combine_clip_visual_v4(mod, arrays)
    assert E.count_parameters(mod) == sum(a.size for a in arrays)
    clip = [rng.standard_normal((n, 64)), rng.standard_normal((n, 5, 7, 16)), rng.standard_normal((n, 4, 4, 32)),
            rng.standard_normal((n, 3, 2, 32)), rng.standard_normal((n, 2, 3, 64))]                  # pooled + NHWC stage maps
    visual, text = rng.standard_normal((n, *half, 32)), rng.standard_normal((n, 64))
    nchw = lambda a: torch.from_numpy(a).permute(0, 3, 1, 2)
    with torch.no_grad():
        got = mod((torch.from_numpy(clip[0]), *map(nchw, clip[1:])), nchw(visual), torch.from_numpy(text))
    assert got.shape == (n, 256, 16, 32)
    ref = R.combine_clip_visual_v4_ref(arrays, clip, visual, text, half, activation, use_dense)
    err = np.abs(got.permute(0, 2, 3, 1).numpy() - ref).max() / np.abs(ref).max()
    assert err < 1e-12, err
    # a wrong shape raises and names the variable; so does a wrong count
    bad = list(arrays)
    bad[-1] = np.zeros((1, 1, 256, 48), np.float32)
    with pytest.raises(ValueError, match='conv_fusion_3.conv'):
        E.load_combine_clip_visual_v4(mod, bad)
    with pytest.raises(ValueError, match='variables'):
        E.load_combine_clip_visual_v4(mod, arrays[:-1])


def test_gradients_reach_the_fusion_through_torch():
    torch.manual_seed(1)
    mod = E.CombineCLIPVisualV4(use_dense=True, activation='elu', half_size=(8, 8), visual_channels=32, **TINY_FUSION)      # fused_tail='auto'
    clip = (torch.randn(1, 64), torch.randn(1, 16, 4, 4), torch.randn(1, 32, 2, 2), torch.randn(1, 32, 2, 2), torch.randn(1, 64, 1, 1))
    out = mod(clip, torch.randn(1, 32, 8, 8), torch.randn(1, 64))
    out.square().mean().backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in mod.parameters())
    mod.fused_tail = True
    with pytest.raises(RuntimeError, match='no backward'):
        mod(clip, torch.randn(1, 32, 8, 8), torch.randn(1, 64))
    with pytest.raises(ValueError):
        E.CombineCLIPVisualV4(activation='gelu')


@pytest.mark.parametrize('shape', R.TAIL_SHAPES, ids=str)
def test_tail_reference_against_torch(shape):
    a, b, weight = R.tail_inputs(shape)
    ref = R.tail_ref(a, b, weight, shape[5])
    assert ref.shape == (shape[0], 2 * shape[1], 2 * shape[2], 256)
    got = R.torch_tail(a, b, weight, shape[5], torch.float64)
    assert R.rel_l2(got, ref) < 1e-14 and R.worst(got, ref) < 1e-14
    # the up-sampling as csrc/feature_tail.hip states it: taps clamp((Y - 1) >> 1), + 1; weights (3/4, 1/4) for odd Y, (1/4, 3/4) for even Y
    h = shape[1]
    y = np.concatenate([a, b], -1).astype(np.float64)[..., :3]
    up = R.resize_bilinear(y, (2 * h, 2 * shape[2]))
    for Y in range(2 * h):
        r0, r1 = np.clip(((Y - 1) >> 1, ((Y - 1) >> 1) + 1), 0, h - 1)
        w0, w1 = (0.75, 0.25) if Y % 2 else (0.25, 0.75)
        rows = w0 * y[:, r0] + w1 * y[:, r1]
        assert np.abs(R.resize_bilinear(rows[:, None], (1, 2 * shape[2]))[:, 0] - up[:, Y]).max() < 1e-14


MISTAKES = ['align_corners', 'zero_padding', 'act_after_conv', 'swapped', 'relu_for_elu', 'reversed_weight']


@pytest.mark.parametrize('shape', R.TAIL_SHAPES, ids=str)
def test_planted_mistakes_are_far_above_the_gpu_bar(shape):
    """Each wrong reading of the tail differs from the right one by far more than the GPU test allows (8 x the float32 torch run's error,
    about 2e-6): the bar can tell them apart.  Where a mistake is no mistake - no activation to misplace, a 1 x 1 image whose corners
    ARE its centre - the case is skipped by construction, not by tolerance."""
    a, b, weight = R.tail_inputs(shape)
    act = shape[5]
    ref = R.tail_ref(a, b, weight, act)
    e32_l2, e32_worst = R.float32_tail_error(shape)
    assert 2e-8 < e32_l2 < 1e-6 and 5e-8 < e32_worst < 5e-6, (e32_l2, e32_worst)          # fp32 rounding level, not 0 and not loose
    for mistake in MISTAKES:
        if (mistake == 'act_after_conv' and act is None) or (mistake == 'relu_for_elu' and act != 'elu'):
            continue
        if mistake == 'align_corners' and shape[1] == 1 and shape[2] == 1:
            continue
        wrong = R.tail_ref(a, b, weight, act, mistake=mistake)
        assert R.rel_l2(wrong, ref) > 0.1 > 1000 * R.TAIL_BAR * e32_l2, (mistake, R.rel_l2(wrong, ref))
        assert R.worst(wrong, ref) > 1000 * R.TAIL_BAR * e32_worst, (mistake, R.worst(wrong, ref))


def test_fuse_upsample2x_validates_its_arguments_without_a_gpu():
    lib = _lib.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    call = lambda a=one, b=one, wt=one, n=1, h=4, w=4, ca=128, cb=256, act=2, out=one, bf16=0: lib.mvnerf_fuse_upsample2x(
        a, b, wt, n, h, w, ca, cb, act, out, bf16, None)
    for kw, name in ((dict(a=None), b'(a)'), (dict(b=None), b'(b)'), (dict(wt=None), b'(weight)'), (dict(out=None), b'(out)')):
        assert call(**kw) == -1 and b'null pointer' in lib.mvnerf_last_error() and name in lib.mvnerf_last_error()
    for kw in (dict(n=0), dict(h=0), dict(w=-1)):
        assert call(**kw) == -1
    assert call(ca=24) == -2 and b'Ca=24' in lib.mvnerf_last_error()
    assert call(ca=0) == -2 and call(cb=8) == -2 and b'Cb=8' in lib.mvnerf_last_error()
    assert call(act=3) == -2 and b'act=3' in lib.mvnerf_last_error()
    assert call(act=-1) == -2
    assert call(ca=272, cb=256) == -2 and b'Ca+Cb=528' in lib.mvnerf_last_error()
    for kw, name in ((dict(a=odd), b'a must'), (dict(b=odd), b'b must'), (dict(wt=odd), b'weight must'), (dict(out=odd), b'out must')):
        assert call(**kw) == -3 and name in lib.mvnerf_last_error()
    assert call(ca=24, a=odd) == -2                                                      # the shape is checked before the alignment


def test_ops_wrapper_has_no_cpu_path():
    from thesis_clip_nerf_amd import ops
    with pytest.raises(ValueError, match='no CPU path'):
        ops.fuse_upsample2x(torch.zeros(1, 2, 2, 16), torch.zeros(1, 2, 2, 16), torch.zeros(32, 256), 'elu')
    mod = E.CombineCLIPVisualV0((2, 2), 16, 16, 256, fused_tail=True)
    with torch.no_grad(), pytest.raises(ValueError, match='no CPU path'):
        mod(torch.zeros(1, 16, 2, 2), torch.zeros(1, 16, 2, 2))


def test_tokenize_is_deterministic_and_clip_shaped():
    t = E.tokenize(['Pick up the red block.', 'pick up the red block .', 'put the blue mug into the green bowl'])
    assert t.shape == (3, 77) and t.dtype == np.int32
    assert np.array_equal(t[0], t[1]) and not np.array_equal(t[0], t[2])                  # case and spacing do not matter, words do
    assert t[0, 0] == 49406 and t[0, 7] == 49407 and not t[0, 8:].any() and (t >= 0).all() and t.max() < 49408
    assert np.array_equal(E.tokenize('pick up the red block.'), t[:1])
    assert t[0, 1] == 28584 and t[0, 3] == 10944                                          # crc32 of 'pick', 'the': the same ids in every process
    with pytest.raises(RuntimeError):
        E.tokenize('word ' * 80)
    text = E.SyntheticCLIPText(embed_dim=64)
    e = text(t)
    assert e.shape == (3, 64) and torch.equal(e[0], e[1]) and not torch.equal(e[0], e[2])
    assert torch.allclose(e.pow(2).mean(1), torch.ones(3), atol=1e-5)
    swapped = text(E.tokenize('block red the up pick.'))
    assert not torch.allclose(swapped, e[:1])                                             # word order counts


def _batch(dataset, with_tokens, **kw):
    np.random.seed(7)
    gen = T.LanguageDataGenerator(dataset, BOUNDS, n_views=2, batch_size=2, shuffle=True, pose_augmentation_factor=4, n_future_poses=3,
                                  rotation_representation='6d', **({'with_tokens': True} if with_tokens else {}), **kw)
    return gen[0], gen.indices[:2]


def test_generator_tokens_are_optional_and_change_nothing_else():
    ds = T.SyntheticLanguageDataset(n_scenes=3, n_perspectives=5, height=8, width=12, seed=5)
    ((inputs, features), labels), _ = _batch(ds, False)
    assert len(inputs) == 8 and inputs[7] is None
    enc = T.EncodedLanguageDataset(ds, producer=None)                     # (the producer is only run by feature_map)
    assert enc.n_perspectives == 5 and len(enc) == 3 and enc.tokens(1).shape == (77,) and enc.tokens(1).dtype == np.int32
    assert np.array_equal(enc.tokens(1), E.tokenize(ds.instruction(1))[0])
    assert len({ds.instruction(i) for i in range(3)}) == 3 and isinstance(ds.instruction(0), str)
    enc.feature_map = ds.feature_map                                      # the bump map: only the tokens differ from the plain batch
    ((inputs_t, features_t), labels_t), order = _batch(enc, True)
    assert inputs_t[7].shape == (2, 77) and inputs_t[7].dtype == np.int32
    assert np.array_equal(inputs_t[7], np.stack([enc.tokens(i) for i in order]))
    for x, y in zip((*inputs[:7], features, *labels), (*inputs_t[:7], features_t, *labels_t)):
        assert np.array_equal(x, y)
    assert T.get_inputs(ds, 1, 3)[0][3] is None
    data = T.get_inputs(enc, 1, 3, with_tokens=True)[0]
    assert data[3].shape == (1, 77) and data[3].dtype == np.int32 and np.array_equal(data[3][0], enc.tokens(1))


def test_encoded_dataset_runs_the_producer_on_the_scene_instruction():
    torch.manual_seed(2)
    ds = T.SyntheticLanguageDataset(n_scenes=2, n_perspectives=5, height=32, width=32, seed=5)
    prod = tiny_producer()
    enc = T.EncodedLanguageDataset(ds, prod)
    fm = enc.feature_map(1, 2)
    assert isinstance(fm, np.ndarray) and fm.shape == (32, 32, 256) and fm.dtype == np.float32
    image = torch.from_numpy((ds.colors[1][2] / 255.0).astype(np.float32))[None]
    assert np.array_equal(fm, prod(image, tokens=E.tokenize([ds.instruction(1)])).numpy()[0])
    other = enc.feature_map(1, 2, instruction='pick up the blue mug')
    assert R.rel_l2(other, fm) > 1e-3                                     # the instruction reaches the map
    ((inputs, features), labels), _ = _batch(enc, True)
    assert features.shape == (2, 2, 32, 32, 256) and features.dtype == np.float32 and inputs[7].shape == (2, 77)
