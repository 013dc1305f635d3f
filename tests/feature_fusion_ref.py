"""Float64 references of the language fusion, written from the Keras semantics (NHWC tensors, HWIO convolution kernels, Dense kernels
(in, out); src/lib/mvnerf/layers.py:414-520, 593-660) and not by calling thesis_clip_nerf_amd.encoders:

* :func:`tail_ref` - the tail both feature producers end with, ConvFusion + UpSampling2D(2, bilinear): what csrc/feature_tail.hip fuses.
  `mistake=` plants one wrong reading of it, for the test that each of them is far above the GPU bar.
* :func:`combine_clip_visual_v4_ref` - the whole CombineCLIPVisualV4 from the 13 (or 10) Keras variables in `model.weights` order.

Also the shapes, inputs and the bar of the GPU test of the fused tail, shared with its CPU companion (tests/test_feature_fusion_cpu.py)."""
import numpy as np

# (N, h, w, Ca, Cb, act): more than one 7 x 15 tile each way with ragged edges, images thinner than a tile, every activation, both channel splits
TAIL_SHAPES = [(2, 9, 11, 128, 256, 'elu'), (1, 9, 11, 256, 256, None), (1, 3, 17, 128, 256, 'elu'), (1, 17, 2, 256, 256, 'relu'),
               (1, 1, 1, 16, 16, 'relu')]
TAIL_BAR = 8.0          # e64 of the kernel <= TAIL_BAR x e64 of the float32 torch run of the same tail (relative L2, and worst element)


def tail_inputs(shape, seed=0):
    """Seeded unit normals a (N,h,w,Ca), b (N,h,w,Cb) and the weight (Ca+Cb, 256) / sqrt(Ca+Cb), float32."""
    n, h, w, ca, cb, _ = shape
    rng = np.random.default_rng([seed, n, h, w, ca, cb])
    a = rng.standard_normal((n, h, w, ca)).astype(np.float32)
    b = rng.standard_normal((n, h, w, cb)).astype(np.float32)
    weight = (rng.standard_normal((ca + cb, 256)) / np.sqrt(ca + cb)).astype(np.float32)
    return a, b, weight


def activation(x, name):
    if name is None:
        return x
    if name == 'relu':
        return np.maximum(x, 0.0)
    if name == 'elu':
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    raise ValueError(name)


def _axis_taps(n_in, n_out, align_corners=False):
    """Bilinear taps along one axis -> (i0, i1, lam): out = (1 - lam) in[i0] + lam in[i1].  Half-pixel centres, the source
    coordinate clamped at 0 and the upper tap at the last sample (tf.image.resize / UpSampling2D / Resizing, bilinear, no antialias)."""
    o = np.arange(n_out, dtype=np.float64)
    if align_corners:
        src = o * ((n_in - 1) / (n_out - 1)) if n_out > 1 else np.zeros(n_out)
    else:
        src = np.maximum((o + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def resize_bilinear(x, size, align_corners=False):
    """x (N, h, w, C) float64 -> (N, size[0], size[1], C)."""
    r0, r1, lr = _axis_taps(x.shape[1], size[0], align_corners)
    c0, c1, lc = _axis_taps(x.shape[2], size[1], align_corners)
    rows = x[:, r0] * (1.0 - lr)[None, :, None, None] + x[:, r1] * lr[None, :, None, None]
    return rows[:, :, c0] * (1.0 - lc)[None, None, :, None] + rows[:, :, c1] * lc[None, None, :, None]


def upsample2x_zero_padded(y):
    """The x2 up-sampling with taps outside the image read as 0 instead of clamped (a planted mistake)."""
    n, h, w, c = y.shape
    p = np.zeros((n, h + 2, w + 2, c))
    p[:, 1:-1, 1:-1] = y
    out = np.zeros((n, 2 * h, 2 * w, c))
    for dy in range(2):
        for dx in range(2):
            # output (2 m + dy, 2 k + dx): rows m - 1 + dy, m + dy with weights (1/4, 3/4) for dy = 0 and (3/4, 1/4) for dy = 1
            wy, wx = ((0.25, 0.75), (0.75, 0.25))[dy], ((0.25, 0.75), (0.75, 0.25))[dx]
            acc = 0.0
            for iy in range(2):
                for ix in range(2):
                    acc = acc + wy[iy] * wx[ix] * p[:, dy + iy:dy + iy + h, dx + ix:dx + ix + w]
            out[:, dy::2, dx::2] = acc
    return out


def tail_ref(a, b, weight, act, mistake=None):
    """UpSampling2D(2, bilinear)(Conv2D(256, 1, use_bias=False)(act(concat([a, b], -1)))) in float64, NHWC; weight (Ca+Cb, 256)."""
    a, b, weight = (np.asarray(t, dtype=np.float64) for t in (a, b, weight))
    if mistake == 'swapped':
        x = np.concatenate([b, a], -1)
    else:
        x = np.concatenate([a, b], -1)
    if mistake == 'reversed_weight':
        weight = weight[::-1]
    if mistake == 'relu_for_elu':
        act = 'relu'
    if mistake == 'act_after_conv':
        y = activation(x @ weight, act)
    else:
        y = activation(x, act) @ weight
    size = (2 * y.shape[1], 2 * y.shape[2])
    if mistake == 'zero_padding':
        return upsample2x_zero_padded(y)
    return resize_bilinear(y, size, align_corners=mistake == 'align_corners')


def rel_l2(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm((x - ref).ravel()) / np.linalg.norm(ref.ravel()))


def worst(x, ref):
    """The worst element's error relative to the largest reference magnitude."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def torch_tail(a, b, weight, act, dtype):
    """The torch tail the fused pass replaces (cat -> act -> conv -> interpolate), on the CPU in `dtype` -> NHWC array."""
    import torch
    import torch.nn.functional as F
    ta, tb, tw = (torch.from_numpy(np.ascontiguousarray(t)).to(dtype) for t in (a, b, weight))
    x = torch.cat([ta, tb], -1).permute(0, 3, 1, 2)
    x = {None: lambda t: t, 'relu': F.relu, 'elu': F.elu}[act](x)
    y = F.conv2d(x, tw.t().reshape(tw.shape[1], tw.shape[0], 1, 1))
    return F.interpolate(y, scale_factor=2, mode='bilinear', align_corners=False).permute(0, 2, 3, 1).contiguous().numpy()


_float32_errors = {}


def float32_tail_error(shape, seed=0):
    """(relative L2, worst element) of the float32 torch run of the tail against :func:`tail_ref`, once per shape."""
    key = (tuple(shape), seed)
    if key not in _float32_errors:
        a, b, weight = tail_inputs(shape, seed)
        ref = tail_ref(a, b, weight, shape[5])
        got = torch_tail(a, b, weight, shape[5], __import__('torch').float32)
        _float32_errors[key] = (rel_l2(got, ref), worst(got, ref))
    return _float32_errors[key]


# ---- the whole fusion -----------------------------------------------------------------------------------------------------------------
def conv2d_same(x, kernel):
    """Conv2D(padding='same', strides 1, use_bias=False): x (N, h, w, Cin), kernel HWIO (kh, kw, Cin, Cout), odd kh, kw."""
    kh, kw = kernel.shape[:2]
    ph, pw = kh // 2, kw // 2
    n, h, w, _ = x.shape
    p = np.zeros((n, h + 2 * ph, w + 2 * pw, x.shape[3]))
    p[:, ph:ph + h, pw:pw + w] = x
    out = np.zeros((n, h, w, kernel.shape[3]))
    for dy in range(kh):
        for dx in range(kw):
            out += p[:, dy:dy + h, dx:dx + w] @ kernel[dy, dx]
    return out


def combine_clip_visual_v4_ref(arrays, clip_outputs, visual_features, clip_textuals, half_size, activation_name='elu', use_dense=True):
    """CombineCLIPVisualV4.call (layers.py:632-660) in float64.  arrays: `model.weights` order (attribute order of __init__); clip_outputs =
    (pooled, l1, l2, l3, l4) NHWC; visual_features (N, h, w, C) NHWC at half_size; clip_textuals (N, T) -> (N, 2h, 2w, filters) NHWC."""
    it = iter(np.asarray(t, dtype=np.float64) for t in arrays)
    f64 = lambda t: np.asarray(t, dtype=np.float64)
    act = lambda t: activation(t, activation_name)
    _, l1, l2, l3, l4 = (f64(t) for t in clip_outputs)
    vis, text = f64(visual_features), f64(clip_textuals)
    hh, hw = half_size
    size_1, size_2, size_3 = (hh // 2, hw // 2), (hh // 4, hw // 4), (hh // 8, hw // 8)

    def multiply_fusion(x):
        t = text @ next(it) if use_dense else text[:, :x.shape[3]]            # Tile: Dense(filters, use_bias=False) | Slice
        return x * t[:, None, None, :]

    def up(x, clip_x, shape):
        x = np.concatenate([resize_bilinear(x, (2 * x.shape[1], 2 * x.shape[2])), resize_bilinear(clip_x, shape)], -1)
        x = act(conv2d_same(x, next(it)))
        return act(conv2d_same(x, next(it)))

    def conv_fusion(x1, x2):
        return conv2d_same(act(np.concatenate([x1, x2], -1)), next(it))

    vis_1, vis_2 = resize_bilinear(vis, size_1), resize_bilinear(vis, size_2)
    x = act(conv2d_same(resize_bilinear(l4, size_3), next(it)))
    x = multiply_fusion(x)
    x = up(x, l3, size_2)
    x = multiply_fusion(x)
    x = conv_fusion(x, vis_2)
    x = up(x, l2, size_1)
    x = multiply_fusion(x)
    x = conv_fusion(x, vis_1)
    x = up(x, l1, (hh, hw))
    x = conv_fusion(x, vis)
    assert next(it, None) is None, 'unused variables'
    return resize_bilinear(x, (2 * hh, 2 * hw))
