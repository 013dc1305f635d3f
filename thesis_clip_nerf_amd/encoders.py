"""Feature-map producer in front of the render hot path: PyTorch-ROCm modules with the structure of the
reference's `VisualFeatures` (src/lib/mvnerf/layers.py:232-259: conv encoder :36-57 + ViT-B/16 with a DPT-style decoder
:60-229) and `CombineCLIPVisualV0` (src/lib/mvnerf/legacy_layers.py:154-191), emitting `combined_features`
(B, V, H, W, 256) NHWC - contiguous, fp32 or bf16 - i.e. exactly the layout `mvnerf_project_texels` / the gather read,
and a Keras-variable importer that takes plain arrays (no TensorFlow needed here).

What is and is not reproduced:
* layer structure, shapes, paddings (TensorFlow 'same' with stride 2 pads more at the END), Keras defaults
  (BatchNormalization eps 1e-3 / momentum 0.99, LayerNormalization eps 1e-3, exact-erf gelu, glorot / zeros init) and the
  reference's quirks: `Block` applies ONE BatchNormalization to both convolutions and always in training mode
  (layers.py:10-14,22,26), the transformer block's first norm is a BatchNormalization over the embedding axis and its second
  residual adds the block INPUT (layers.py:76,88-94).  Parity unpinned: TensorFlow is not available and the reference ships
  no fixtures for these layers; the restated numerics are checked for shape / layout / gradient flow only.
* CLIP RN50 (`clip_visual`, an external frozen SavedModel whose weights are not available offline) is NOT rebuilt: its
  stage-1 map (B, 56, 56, 256) is an input of :class:`CombineCLIPVisualV0`; :class:`SyntheticCLIPStage1` is a frozen random
  stand-in for synthetic runs.
* Sizes are constructor arguments (the reference hard-codes 480x640 / 224 / ViT-B): tests run a tiny configuration.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn


def _same_pad(size, k, s):
    """TensorFlow 'same' padding for one spatial axis: (before, after)."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


class SameConv2d(nn.Conv2d):
    """Conv2D(padding='same') with TensorFlow's asymmetric padding when the stride is > 1.  Keras init: glorot_uniform, zeros."""

    def __init__(self, c_in, c_out, k, stride=1, bias=True):
        super().__init__(c_in, c_out, k, stride=stride, padding=0, bias=bias)
        nn.init.xavier_uniform_(self.weight)
        if bias:
            nn.init.zeros_(self.bias)

    def forward(self, x):
        ph = _same_pad(x.shape[2], self.kernel_size[0], self.stride[0])
        pw = _same_pad(x.shape[3], self.kernel_size[1], self.stride[1])
        return super().forward(F.pad(x, (pw[0], pw[1], ph[0], ph[1])))


def _keras_bn(c):
    return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)          # Keras momentum 0.99 = torch momentum 0.01


def _check_switch(value, name='fused_conv'):
    if not (value is True or value is False or (isinstance(value, str) and value == 'auto')):      # (1 == True, but the code asks `is True`)
        raise ValueError(f"{name}: {value!r}, expected True, False or 'auto'")
    return value


def _check_bool(value, name='fused_backward'):
    if not (value is True or value is False):
        raise ValueError(f'{name}: {value!r}, expected True or False')
    return value


class Block(nn.Module):
    """layers.py:7-33.  One BatchNormalization serves both convolutions (the attribute is assigned twice in the reference)
    and it always normalises with batch statistics (`training=True` is hard-coded there).
    fused_conv (default False: torch): each convolution as ops.conv3x3 (bias, tile statistics) -> ops.bn_finalize -> ops.bn_apply
    (skip, relu) under the rule of :func:`_wants_fused`, see :func:`conv3x3_bn`; the downsample branch stays torch.
    fused_backward (default False): where a call under `fused_conv` needs a gradient, the convolutions run as the differentiable HIP
    pass (:class:`Conv3x3BiasFunction`) and the normalisation, skip and relu as torch, instead of torch all over ('auto') or the
    "no backward" error (True)."""

    def __init__(self, c_in, n_features, downsample=None, fused_conv=False, fused_backward=False):
        super().__init__()
        self.conv_1 = SameConv2d(c_in, n_features, 3)
        self.conv_2 = SameConv2d(n_features, n_features, 3)
        self.norm_1 = _keras_bn(n_features)
        self.downsample = downsample
        self.fused_conv = fused_conv
        self.fused_backward = fused_backward

    @property
    def fused_conv(self):
        return self._fused_conv

    @fused_conv.setter
    def fused_conv(self, value):
        self._fused_conv = _check_switch(value)

    @property
    def fused_backward(self):
        return self._fused_backward

    @fused_backward.setter
    def fused_backward(self, value):
        self._fused_backward = _check_bool(value)

    def _norm(self, x):
        return F.batch_norm(x, None, None, self.norm_1.weight, self.norm_1.bias, True, 0.0, self.norm_1.eps)

    def run(self, x, amax=None):
        """-> (out, amax | None): amax bounds |x| (a device float, or None), the returned one is max |out| when conv_2 ran fused."""
        skip = x if self.downsample is None else self.downsample(x)
        out, amax = conv3x3_bn(self.conv_1, self.norm_1, x, None, self.fused_conv, amax, self.fused_backward)
        return conv3x3_bn(self.conv_2, self.norm_1, out, skip, self.fused_conv, amax, self.fused_backward)

    def forward(self, x):
        if self.fused_conv is False:
            skip = x if self.downsample is None else self.downsample(x)
            out = F.relu(self._norm(self.conv_1(x)))
            out = self._norm(self.conv_2(out))
            return F.relu(out + skip)
        return self.run(x)[0]


class ConvolutionalEncoder(nn.Module):
    """layers.py:36-57: 7x7/2 conv -> BN -> ReLU -> 3 residual blocks of n_features / 2 channels; (H, W) -> (H/2, W/2).
    fused_conv (default False): handed to the three blocks, every apply's amax_out the next convolution's amax; the stem stays torch.
    fused_backward (default False): handed to the three blocks too."""

    def __init__(self, n_features=256, stem=64, fused_conv=False, fused_backward=False):
        super().__init__()
        half = n_features // 2
        downsample = nn.Sequential(SameConv2d(stem, half, 1, bias=False), _keras_bn(half))
        self.conv_features = nn.Sequential(SameConv2d(3, stem, 7, stride=2, bias=False), _keras_bn(stem), nn.ReLU(),
                                           Block(stem, half, downsample), Block(half, half), Block(half, half))
        self.fused_conv = fused_conv
        self.fused_backward = fused_backward

    @property
    def fused_conv(self):
        return self._fused_conv

    @fused_conv.setter
    def fused_conv(self, value):
        self._fused_conv = _check_switch(value)
        for block in self.conv_features[3:]:
            block.fused_conv = value

    @property
    def fused_backward(self):
        return self._fused_backward

    @fused_backward.setter
    def fused_backward(self, value):
        self._fused_backward = _check_bool(value)
        for block in self.conv_features[3:]:
            block.fused_backward = value

    def forward(self, x):
        if self.fused_conv is False:
            return self.conv_features(x)
        x, amax = self.conv_features[:3](x), None
        for block in self.conv_features[3:]:
            x, amax = block.run(x, amax)
        return x


class KerasMHA(nn.Module):
    """tf.keras.layers.MultiHeadAttention(num_heads, key_dim = value_dim = embed / heads) on (x, x): biased q/k/v/out projections."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.h, self.d = num_heads, embed_dim // num_heads
        self.q = nn.Linear(embed_dim, self.h * self.d)
        self.k = nn.Linear(embed_dim, self.h * self.d)
        self.v = nn.Linear(embed_dim, self.h * self.d)
        self.o = nn.Linear(self.h * self.d, embed_dim)
        for lin in (self.q, self.k, self.v, self.o):
            nn.init.xavier_uniform_(lin.weight)
            nn.init.zeros_(lin.bias)

    def forward(self, x):
        b, n, _ = x.shape
        split = lambda t: t.view(b, n, self.h, self.d).transpose(1, 2)
        out = F.scaled_dot_product_attention(split(self.q(x)), split(self.k(x)), split(self.v(x)))      # softmax(q k^T / sqrt(d)) v
        return self.o(out.transpose(1, 2).reshape(b, n, self.h * self.d))


class TransformerBlock(nn.Module):
    """layers.py:72-95, quirks kept: the first norm is a BatchNormalization over the embedding axis; `x = inputs + attn`,
    then `inputs + mlp(LayerNorm(x))` - the second residual adds the block input, not x.
    fused_vit (default False: torch): the block as seven HIP launches, see :func:`transformer_block_fused` - under the rule of
    :func:`_wants_fused` and only in eval mode (the first norm then reads its running statistics) and for sizes the kernels take
    (:func:`vit_block_unfusable`); otherwise 'auto' runs torch and True raises."""

    def __init__(self, num_heads=12, embed_dim=768, mlp_ratio=4, fused_vit=False):
        super().__init__()
        self.fused_vit = fused_vit
        self.layer_norm_1 = nn.BatchNorm1d(embed_dim, eps=1e-3, momentum=0.01)
        self.attention = KerasMHA(embed_dim, num_heads)
        self.layer_norm_2 = nn.LayerNorm(embed_dim, eps=1e-3)
        self.dense_0 = nn.Linear(embed_dim, embed_dim * mlp_ratio)
        self.dense_1 = nn.Linear(embed_dim * mlp_ratio, embed_dim)
        for lin in (self.dense_0, self.dense_1):
            nn.init.xavier_uniform_(lin.weight)
            nn.init.zeros_(lin.bias)

    @property
    def fused_vit(self):
        return self._fused_vit

    @fused_vit.setter
    def fused_vit(self, value):
        self._fused_vit = _check_switch(value, 'fused_vit')

    def forward(self, inputs):
        if self.fused_vit is not False and _wants_fused(self.fused_vit, inputs, *self.parameters(), name='fused_vit'):
            reason = vit_block_unfusable(self, inputs)
            if reason is None:
                return transformer_block_fused(self, inputs, self.fused_vit)
            if self.fused_vit is True:
                raise ValueError(f"fused_vit=True: {reason}; use 'auto'")
        x = self.layer_norm_1(inputs.transpose(1, 2)).transpose(1, 2)
        x = inputs + self.attention(x)
        x = self.layer_norm_2(x)
        return inputs + self.dense_1(F.gelu(self.dense_0(x)))


class VisionTransformer(nn.Module):
    """layers.py:98-157 (skip_classification=True): patch embedding, class token, learned positions, `sum(hooks)`-free grouping of
    the blocks at the hook depths; returns the token maps after each group.
    fused_vit (default False): handed to every block; patch embedding, class token and position add stay torch."""

    def __init__(self, img_size=(224, 224), patch_size=16, embed_dim=768, mlp_ratio=4, hooks=(3, 6, 9, 12), num_heads=12, fused_vit=False):
        super().__init__()
        self.grid_size = (img_size[0] // patch_size, img_size[1] // patch_size)
        self.patch_embed = nn.Conv2d(3, embed_dim, patch_size, stride=patch_size)
        nn.init.xavier_uniform_(self.patch_embed.weight)
        nn.init.zeros_(self.patch_embed.bias)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embedding = nn.Parameter(0.02 * torch.randn(1, self.grid_size[0] * self.grid_size[1] + 1, embed_dim))
        depth = [hooks[0]] + [hooks[i] - hooks[i - 1] for i in range(1, len(hooks))]
        self.transformer_blocks = nn.ModuleList(
            nn.Sequential(*[TransformerBlock(num_heads, embed_dim, mlp_ratio) for _ in range(d)]) for d in depth)
        self.fused_vit = fused_vit

    @property
    def fused_vit(self):
        return self._fused_vit

    @fused_vit.setter
    def fused_vit(self, value):
        self._fused_vit = _check_switch(value, 'fused_vit')
        for blocks in self.transformer_blocks:
            for block in blocks:
                block.fused_vit = value

    def forward(self, x):
        x = self.patch_embed(x).flatten(2).transpose(1, 2)                     # b (h w) c
        x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], 1) + self.pos_embedding
        feats = []
        for blocks in self.transformer_blocks:
            x = blocks(x)
            feats.append(x)
        return feats


def _up(x, s):
    return F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=False)     # UpSampling2D(interpolation='bilinear')


def _resize(x, size):
    return F.interpolate(x, size=size, mode='bilinear', align_corners=False)          # Resizing(interpolation='bilinear')


class VisionTransformerEncoder(nn.Module):
    """layers.py:160-229: four token maps -> post-processing to 4 / 2 / 1 / 0.5 x the patch grid -> 3x3 decode convs to
    n_features -> bilinear up-sampling to 8 x the grid -> concat -> ReLU, conv, ReLU, conv to n_features / 2.
    fused_conv (default False: torch): under the rule of :func:`_wants_fused` both `output_conv` convolutions run as ops.conv3x3 with
    act_in = relu and their bias, and each `conv_decode` whose channel counts the kernel takes (multiples of 32 -> 64; at the reference's
    sizes all but the first, 48 -> 256) as a plain ops.conv3x3 - under 'auto' only where the launch is large enough to beat the torch
    path (:func:`conv3x3_auto_pays`); the others and the post-processing stay torch.
    fused_vit (default False), a switch of its own: the transformer blocks of the ViT as HIP launches (:class:`TransformerBlock`).
    fused_backward (default False): where a call under `fused_conv` needs a gradient, the same convolutions as the differentiable HIP
    pass (:class:`Conv3x3BiasFunction`; `conv_decode` under 'auto' keeps its workgroup rule)."""

    def __init__(self, img_size=(224, 224), patch_size=16, embed_dim=768, n_features=256, mlp_ratio=4, hooks=(3, 6, 9, 12),
                 features=(48, 96, 192, 384), num_heads=12, fused_conv=False, fused_vit=False, fused_backward=False):
        super().__init__()
        self.fused_conv = fused_conv
        self.fused_backward = fused_backward
        self.vit = VisionTransformer(img_size, patch_size, embed_dim, mlp_ratio, hooks, num_heads, fused_vit)
        f = features

        def convT(c, k):
            m = nn.ConvTranspose2d(c, c, k, stride=k)
            nn.init.xavier_uniform_(m.weight)
            nn.init.zeros_(m.bias)
            return m
        self.post_process_1 = nn.Sequential(SameConv2d(embed_dim, f[0], 1), convT(f[0], 4))
        self.post_process_2 = nn.Sequential(SameConv2d(embed_dim, f[1], 1), convT(f[1], 2))
        self.post_process_3 = SameConv2d(embed_dim, f[2], 1)
        self.post_process_4 = nn.Sequential(SameConv2d(embed_dim, f[3], 1), SameConv2d(f[3], f[3], 3, stride=2))
        self.conv_decode = nn.ModuleList(SameConv2d(c, n_features, 3, bias=False) for c in f)
        self.output_conv = nn.Sequential(nn.ReLU(), SameConv2d(4 * n_features, n_features, 3), nn.ReLU(),
                                         SameConv2d(n_features, n_features // 2, 3))

    @property
    def fused_conv(self):
        return self._fused_conv

    @fused_conv.setter
    def fused_conv(self, value):
        self._fused_conv = _check_switch(value)

    @property
    def fused_backward(self):
        return self._fused_backward

    @fused_backward.setter
    def fused_backward(self, value):
        self._fused_backward = _check_bool(value)

    @property
    def fused_vit(self):
        return self.vit.fused_vit

    @fused_vit.setter
    def fused_vit(self, value):
        self.vit.fused_vit = value

    def forward(self, x):
        gh, gw = self.vit.grid_size
        feats = [t[:, 1:].transpose(1, 2).reshape(t.shape[0], -1, gh, gw) for t in self.vit(x)]
        post = (self.post_process_1, self.post_process_2, self.post_process_3, self.post_process_4)
        if self.fused_conv is False:
            maps = [_up(dec(pp(t)), s) for t, pp, dec, s in zip(feats, post, self.conv_decode, (2, 4, 8, 16))]
            return self.output_conv(torch.cat(maps, 1))
        maps = []
        for t, pp, dec, s in zip(feats, post, self.conv_decode, (2, 4, 8, 16)):
            t = pp(t)
            # (True is about gradients and devices, not channel counts; 'auto' also leaves launches too small to pay to torch)
            takes = conv3x3_fusable(dec, t.shape[1]) and (self.fused_conv is True or conv3x3_auto_pays(t.shape[0], *t.shape[2:], dec.out_channels))
            switch = self.fused_conv if takes else False
            if switch is not False and _wants_fused_backward(switch, self.fused_backward, dec.weight, t):
                maps.append(_up(conv3x3_bias(dec, t, None, switch, None, True)[0], s))
            else:
                maps.append(_up(conv3x3_act(dec, t, None, None, switch)[0], s))
        conv_a, conv_b = self.output_conv[1], self.output_conv[3]
        x, amax = conv3x3_bias(conv_a, torch.cat(maps, 1), 'relu', self.fused_conv, None, self.fused_backward)
        return conv3x3_bias(conv_b, x, 'relu', self.fused_conv, amax, self.fused_backward)[0]


class VisualFeatures(nn.Module):
    """layers.py:232-259: images (N, H, W, 3) in [0, 1] -> (N, H/2, W/2, n_features) = [ViT latents resized | conv features].
    fused_conv: False (default) | True | 'auto' - handed to both encoders: their stride-1 3x3 convolutions and the batch-statistics
    normalisation behind the blocks' as HIP passes when on the GPU and nothing needs a gradient (inference only; see `fused_backward`).
    fused_vit: False (default) | True | 'auto' - the ViT's transformer blocks as HIP passes, eval mode only (:class:`TransformerBlock`).
    fused_backward: False (default) | True - handed to both encoders: with it the stride-1 3x3 convolutions under `fused_conv` stay HIP
    passes where a gradient is needed (training through train_nerf), forward and backward (:class:`Conv3x3BiasFunction`)."""

    def __init__(self, n_features=256, original_image_size=(480, 640), transformer_image_size=(224, 224), fused_conv=False, fused_vit=False,
                 fused_backward=False, **vit_kw):
        super().__init__()
        self.conv_features = ConvolutionalEncoder(n_features)
        self.vision_transformer = VisionTransformerEncoder(img_size=transformer_image_size, n_features=n_features, fused_vit=fused_vit, **vit_kw)
        self.transformer_image_size = tuple(transformer_image_size)
        self.half_size = (original_image_size[0] // 2, original_image_size[1] // 2)
        self.fused_conv = fused_conv
        self.fused_backward = fused_backward

    @property
    def fused_conv(self):
        return self._fused_conv

    @fused_conv.setter
    def fused_conv(self, value):
        self._fused_conv = _check_switch(value)
        self.conv_features.fused_conv = value
        self.vision_transformer.fused_conv = value

    @property
    def fused_backward(self):
        return self._fused_backward

    @fused_backward.setter
    def fused_backward(self, value):
        self._fused_backward = _check_bool(value)
        self.conv_features.fused_backward = value
        self.vision_transformer.fused_backward = value

    @property
    def fused_vit(self):
        return self.vision_transformer.fused_vit

    @fused_vit.setter
    def fused_vit(self, value):
        self.vision_transformer.fused_vit = value

    def forward(self, images_nhwc):
        x = images_nhwc.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        latents = _resize(self.vision_transformer(_resize(x, self.transformer_image_size)), self.half_size)
        return torch.cat([latents, self.conv_features(x)], 1)                  # NCHW view, channels-last storage


# ---- the transformer block as HIP passes (csrc/token_linear.hip, csrc/attention.hip) --------------------------------------
VIT_PASSES = ('linear_qkv', 'attention', 'linear_out', 'layer_norm', 'linear_0', 'linear_1')
# The passes 'auto' leaves to torch inside a fused block: those whose HIP median was above the torch path's at the reference's shape
# (3 x 197 tokens of 768 channels, `dense` / `layer_norm` entries of profiles/vit_bench.json): the QKV projection 0.95x,
# dense_0 0.91x, dense_1 0.66x, the LayerNorm 0.61x; the out projection (1.45x) and the attention (1.44x) were faster in every repeat.
# One shape on one box: other token counts or widths were not measured.  fused_vit=True runs every pass in HIP.
VIT_AUTO_TORCH_PASSES = frozenset({'linear_qkv', 'layer_norm', 'linear_0', 'linear_1'})


def _param_key(*tensors):
    return tuple((t._version, t.data_ptr(), t.device) for t in tensors)


def _loads(*modules):
    return tuple(m.__dict__.get('_mvnerf_loads', 0) for m in modules)


def _mark_loaded(module):
    """A loader wrote `.data` (which does not bump the parameter version the packed caches key on): count it and drop the module's cache."""
    module.__dict__['_mvnerf_loads'] = module.__dict__.get('_mvnerf_loads', 0) + 1
    module.__dict__.pop('_mvnerf_packed', None)
    module.__dict__.pop('_mvnerf_packed_t', None)
    module.__dict__.pop('_mvnerf_packed_t_rows', None)


def _cached(module, key, make):
    cached = module.__dict__.get('_mvnerf_packed')
    if cached is None or cached[0] != key:
        cached = (key, make())
        module.__dict__['_mvnerf_packed'] = cached
    return cached[1]


def _packed_linear(lin):
    """The packed fp16-piece stream of `lin.weight` (ops.linear_pack), cached on the module per parameter version like :func:`_packed_conv3x3`."""
    from . import ops
    return _cached(lin, (_param_key(lin.weight), _loads(lin)), lambda: ops.linear_pack(lin.weight.detach().contiguous()))


def _packed_qkv(mha):
    """(packed stream, bias) of the q, k, v projections of a :class:`KerasMHA` as ONE Dense layer to 3 heads d outputs: the three weights
    and biases concatenated in that order, so the GEMM's output is (tokens, 3, heads, d).  Cached on the module per parameter version."""
    from . import ops
    lins = (mha.q, mha.k, mha.v)
    key = (_param_key(*[t for lin in lins for t in (lin.weight, lin.bias)]), _loads(*lins))

    def make():
        weight = torch.cat([lin.weight.detach() for lin in lins], 0).contiguous()
        return ops.linear_pack(weight), torch.cat([lin.bias.detach() for lin in lins], 0).contiguous()
    return _cached(mha, key, make)


def _running_rstd(bn):
    """1 / sqrt(running_var + eps) of an eval-mode BatchNorm, cached per buffer version."""
    key = (_param_key(bn.running_var), _loads(bn), bn.eps)
    return _cached(bn, key, lambda: torch.rsqrt(bn.running_var.detach().double() + bn.eps).float().contiguous())


def vit_block_unfusable(blk, inputs):
    """None when :func:`transformer_block_fused` takes this block on these inputs, else the reason as a phrase."""
    from . import ops
    mha = blk.attention
    if blk.training:
        return 'the block is in training mode (its first norm would have to update its running statistics; call .eval())'
    if inputs.dim() != 3 or inputs.dtype != torch.float32:
        return f'inputs of shape {tuple(inputs.shape)} and dtype {inputs.dtype} are not float32 (batch, tokens, embed)'
    embed = inputs.shape[2]
    if embed % 64 or mha.h * mha.d != embed or blk.dense_0.out_features % 64:
        return f'embed {embed} with {mha.h} heads and {blk.dense_0.out_features} hidden channels is not in multiples of 64'
    if mha.d not in ops.ATTENTION_HEAD_DIMS:
        return f'head dimension {mha.d} is not one of {ops.ATTENTION_HEAD_DIMS}'
    if not 1 <= inputs.shape[1] <= ops.ATTENTION_MAX_TOKENS or inputs.shape[0] < 1:
        return f'{inputs.shape[1]} tokens are more than the attention pass keeps ({ops.ATTENTION_MAX_TOKENS})'
    return None


def transformer_block_fused(blk, inputs, switch=True):
    """:class:`TransformerBlock` on (batch, tokens, embed) as seven launches, every amax_out the next GEMM's amax_x:
    ops.bn_apply (the first norm with its running statistics) -> ops.linear (q, k, v as one Dense layer) -> ops.attention ->
    ops.linear (out projection + inputs) -> ops.layer_norm (in place) -> ops.linear (dense_0, gelu) -> ops.linear (dense_1 + inputs: the
    reference adds the block input here, layers.py:94).  switch='auto' leaves the passes of VIT_AUTO_TORCH_PASSES to torch."""
    from . import ops
    hip = lambda name: switch is True or name not in VIT_AUTO_TORCH_PASSES
    b, n, e = inputs.shape
    x_in = inputs.detach().contiguous()
    words = torch.zeros(4, dtype=torch.float32, device=x_in.device)            # the four amax words of the block, zeroed in one fill
    word = lambda i: dict(amax_out=words[i:i + 1], amax_zeroed=True)
    bn, mha, ln = blk.layer_norm_1, blk.attention, blk.layer_norm_2
    amax = words[0:1]
    x = ops.bn_apply(x_in, bn.running_mean, _running_rstd(bn), bn.weight.detach(), bn.bias.detach(), **word(0))
    if hip('linear_qkv'):
        packed, bias = _packed_qkv(mha)
        qkv = ops.linear(x, packed, 3 * e, bias=bias, amax_x=amax)
    else:
        qkv = torch.cat([lin(x) for lin in (mha.q, mha.k, mha.v)], -1)
    qkv = qkv.view(b, n, 3, mha.h, mha.d)
    if hip('attention'):
        x, amax = ops.attention(qkv, **word(1)), words[1:2]
    else:
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        x, amax = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(b, n, e), None
    if hip('linear_out'):
        x = ops.linear(x, _packed_linear(mha.o), e, bias=mha.o.bias.detach(), residual=x_in, amax_x=amax)
    else:
        x = x_in + mha.o(x)
    if hip('layer_norm'):
        x, amax = ops.layer_norm(x, ln.weight.detach(), ln.bias.detach(), ln.eps, out=x, **word(2)), words[2:3]
    else:
        x, amax = ln(x), None
    if hip('linear_0'):
        x, amax = ops.linear(x, _packed_linear(blk.dense_0), blk.dense_0.out_features, bias=blk.dense_0.bias.detach(), act='gelu', amax_x=amax,
                             **word(3)), words[3:4]
    else:
        x, amax = F.gelu(blk.dense_0(x)), None
    if hip('linear_1'):
        return ops.linear(x, _packed_linear(blk.dense_1), e, bias=blk.dense_1.bias.detach(), residual=x_in, amax_x=amax)
    return x_in + blk.dense_1(x)


_ACT_CODES = {None: 0, 'relu': 1, 'elu': 2}
_ACT_FNS = {None: lambda x: x, 'relu': F.relu, 'elu': F.elu}


def _wants_fused(fused_tail, *tensors, name='fused_tail'):
    """The switch of a fused pass (`fused_tail`, `fused_conv`): True | False | 'auto' = on the GPU and nothing in the call needs a gradient
    (the fused passes have no backward)."""
    if fused_tail not in (True, False, 'auto'):
        raise ValueError(f"{name}: {fused_tail!r}, expected True, False or 'auto'")
    if fused_tail is False:
        return False
    tensors = [t for t in tensors if t is not None]
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in tensors)
    on_gpu = all(t.is_cuda for t in tensors)
    if fused_tail is True:
        if needs_grad:
            raise RuntimeError(f'{name}=True: the fused {name[6:]} has no backward pass; run under torch.no_grad(), freeze the inputs, '
                               f"or use {name}='auto'")
        return True                                                  # (a CPU tensor fails in ops: there is no CPU path)
    return on_gpu and not needs_grad


def conv_fusion_tail(a, b, conv, activation=None, fused=False, out_dtype=None):
    """`up_sample(conv(act([a | b])))` of NCHW a, b with a bias-free 1x1 `conv` to 256 filters -> (N, 256, 2h, 2w), channels-last storage.
    fused: one ops.fuse_upsample2x call, which writes NHWC in `out_dtype` (fp32 | bf16) directly; else torch (fp32; the caller casts).
    fused='backward': :class:`FuseUpsample2xFunction`, the same launch with a HIP backward (fp32 out)."""
    if not fused:
        return _up(conv(_ACT_FNS[activation](torch.cat([a, b], 1))), 2)
    if fused == 'backward':
        return FuseUpsample2xFunction.apply(a, b, conv.weight, activation)
    from . import ops
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()      # free when the storage is channels-last already
    weight = conv.weight.detach().reshape(conv.out_channels, conv.in_channels).t().contiguous()      # (Cin, 256): the Keras kernel as stored
    out = ops.fuse_upsample2x(nhwc(a), nhwc(b), weight, _ACT_CODES[activation], out_dtype or torch.float32)
    return out.permute(0, 3, 1, 2)


class FuseUpsample2xFunction(torch.autograd.Function):
    """:func:`conv_fusion_tail` as HIP passes in both directions: a, b NCHW, `weight` the (256, Ca + Cb, 1, 1) parameter of
    the bias-free 1x1 convolution, `activation` None | 'relu' | 'elu' -> (N, 256, 2h, 2w) fp32, channels-last storage.
    forward: the ops.fuse_upsample2x launch of the inference path; saves a, b (NHWC) and the weight, nothing else - neither the
    concatenated input nor the low-resolution product.  backward, for g = dL/dout: one ops.fuse_upsample2x_bwd launch that computes only
    the halves `needs_input_grad` asks for.  Where the weight needs a gradient the launch also writes the adjoint of the up-sampling,
    g_low, and dW = act([a | b])^T . g_low runs through the fixed-order ops.gemm_tn (torch's matmul on the same two arrays where its shape
    rule does not hold) - a route for correctness, not for speed: the reference never trains this weight (`combine_clip_visual` is not
    in `FeatureProducer.trainable_parameters()`), and freezing it is the intended use."""

    @staticmethod
    def forward(ctx, a, b, weight, activation):
        from . import ops
        an, bn = _nhwc(a), _nhwc(b)
        out = ops.fuse_upsample2x(an, bn, _tail_weight(weight), _ACT_CODES[activation], torch.float32)
        ctx.save_for_backward(an, bn, weight)
        ctx.activation = activation
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        from . import ops
        an, bn, weight = ctx.saved_tensors
        need_a, need_b, need_w = ctx.needs_input_grad[:3]
        da, db, g_low = ops.fuse_upsample2x_bwd(_nhwc(g), an, bn, _tail_weight(weight), _ACT_CODES[ctx.activation], need_a=need_a, need_b=need_b,
                                                need_g_low=need_w)
        dw = None
        if need_w:
            x = _ACT_FNS[ctx.activation](torch.cat([an, bn], -1)).reshape(-1, an.shape[3] + bn.shape[3])
            low = g_low.reshape(-1, g_low.shape[3])
            if x.shape[0] % 8 == 0 and x.shape[1] % 32 == 0:                  # mvnerf_gemm_tn: M % 8, N % 32, K % 64 (K = 256 here)
                dw = ops.gemm_tn(x, low)
            else:
                dw = x.t() @ low
            dw = dw.t().reshape(weight.shape)                                 # (Cin, 256) -> (256, Cin, 1, 1)
        nchw = lambda t: None if t is None else t.permute(0, 3, 1, 2)
        return nchw(da), nchw(db), dw, None


def _tail_weight(weight):
    """(256, Cin, 1, 1) -> (Cin, 256), the Keras 1x1 kernel as stored (512 KiB at most: copied per call)."""
    return weight.detach().reshape(weight.shape[0], weight.shape[1]).t().contiguous()


def _tail_switch(fused_tail, fused_backward, *tensors):
    """What :func:`conv_fusion_tail` runs: 'backward' where `fused_backward` is on and the call is its case (the switch True | 'auto',
    everything on the GPU, a gradient needed; the Function's output is fp32, so a bf16 `out_dtype` keeps today's path) - else whatever
    :func:`_wants_fused` says, its "no backward" error included."""
    if fused_tail not in (True, False, 'auto'):
        raise ValueError(f"fused_tail: {fused_tail!r}, expected True, False or 'auto'")
    if _wants_fused_backward(fused_tail, fused_backward, *tensors):
        return 'backward'
    return _wants_fused(fused_tail, *tensors)


class CombineCLIPVisualV0(nn.Module):
    """legacy_layers.py:154-191: [resize(clip stage-1 map, (H/2, W/2)) | visual features] -> 1x1 conv (no bias) -> x2 bilinear.
    fused_tail (default False: torch): concat + conv + up-sampling as one HIP pass, see :func:`conv_fusion_tail`.
    fused_backward (default False): where a call under `fused_tail` (True | 'auto') needs a gradient and the output is fp32, the tail runs
    as :class:`FuseUpsample2xFunction` - HIP in both directions - instead of torch ('auto') or the "no backward" error (True)."""

    def __init__(self, half_size=(240, 320), clip_channels=256, visual_channels=256, filters=256, fused_tail=False, fused_backward=False):
        super().__init__()
        self.conv = SameConv2d(clip_channels + visual_channels, filters, 1, bias=False)
        self.half_size = tuple(half_size)
        self.fused_tail = fused_tail
        self.fused_backward = fused_backward

    @property
    def fused_backward(self):
        return self._fused_backward

    @fused_backward.setter
    def fused_backward(self, value):
        self._fused_backward = _check_bool(value)

    def forward(self, clip_256, visual_features, out_dtype=None):
        clip = _resize(clip_256, self.half_size)
        fused = _tail_switch(self.fused_tail, self.fused_backward and out_dtype in (None, torch.float32), clip, visual_features,
                             self.conv.weight)
        return conv_fusion_tail(clip, visual_features, self.conv, None, fused, out_dtype)


class SyntheticCLIPStage1(nn.Module):
    """Frozen random stand-in for the stage-1 output (N, 256, 56, 56) of the CLIP RN50 visual trunk (clip/model.py:21-28; the
    SavedModel and its weights are not available offline).  Not trained, carries no semantics."""

    def __init__(self, channels=256, out_size=(56, 56), seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.register_buffer('w', torch.randn(channels, 3, 7, 7, generator=g) * 0.1)
        self.out_size = tuple(out_size)

    @torch.no_grad()
    def forward(self, x_nchw):
        return F.relu(F.adaptive_avg_pool2d(F.conv2d(x_nchw, self.w, stride=2, padding=3), self.out_size))


class FeatureProducer(nn.Module):
    """`MVVNeRFRenderer.call`'s encoder prologue (model_v0.py:75-86) as one callable: images (N, H, W, 3) in [0, 1] ->
    combined_features (N, H, W, 256), NHWC-contiguous in `out_dtype` (fp32, or bf16 to halve the gather traffic).  Use it as
    `MVVNeRFRenderer(feature_encoder=producer)`; `trainable_parameters()` is the reference's optimizer list for the feature
    side (train_nerf.py:27-32: vision_transformer + conv_features at lr 1e-5; combine_clip_visual is NOT in it)."""

    def __init__(self, original_image_size=(480, 640), n_features=256, clip_stage1=None, out_dtype=torch.float32, **visual_kw):
        super().__init__()
        h, w = original_image_size
        if h % 2 or w % 2:
            raise ValueError('image height and width must be even (the encoders work at half resolution)')
        self.visual_features = VisualFeatures(n_features, original_image_size, **visual_kw)
        self.combine_clip_visual = CombineCLIPVisualV0((h // 2, w // 2), 256, n_features, 256)
        self.clip_stage1 = clip_stage1 if clip_stage1 is not None else SyntheticCLIPStage1()
        self.out_dtype = out_dtype

    def trainable_parameters(self):
        return list(self.visual_features.vision_transformer.parameters()) + list(self.visual_features.conv_features.parameters())

    def forward(self, images_nhwc):
        x = images_nhwc.permute(0, 3, 1, 2)
        visual = self.visual_features(images_nhwc)
        with torch.no_grad():
            clip_256 = self.clip_stage1(x)                                   # frozen (layers.py:550-561)
        fused = self.combine_clip_visual(clip_256, visual)                      # (N, 256, H, W), channels-last storage
        out = fused.permute(0, 2, 3, 1)
        out = out.to(self.out_dtype)
        return out if out.is_contiguous() else out.contiguous()


# ---- the language fusion (layers.py:414-520, 593-660) ------------------------------------------------------------------------
def _activation(name):
    if name not in ('relu', 'elu'):
        raise ValueError(f'activation {name} not supported')
    return _ACT_FNS[name]


def conv3x3_fusable(conv, c_a, c_b=0, bias=False):
    """Whether ops.conv3x3 takes this convolution over [a | b]: 3x3, stride 1, channel counts in multiples of 32 / 32 / 64, and no bias
    unless the caller hands it over (`bias=True`: the paths of VisualFeatures)."""
    return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) and (bias or conv.bias is None) and c_a + c_b == conv.in_channels
            and c_a >= 32 and c_a % 32 == 0 and c_b % 32 == 0 and conv.out_channels % 64 == 0)


def _packed_conv3x3(conv):
    """The packed fp16-piece stream of `conv.weight` (ops.conv3x3_pack), cached on the module per parameter version: an in-place
    update (optimizer step, `copy_`, load_combine_clip_visual_v4) re-packs on the next call.  `load_conv` drops the cache itself."""
    from . import ops
    weight = conv.weight
    key = (weight._version, weight.data_ptr(), weight.device)
    cached = conv.__dict__.get('_mvnerf_packed')
    if cached is None or cached[0] != key:
        cached = (key, ops.conv3x3_pack(weight.detach().permute(2, 3, 1, 0).contiguous()))      # HWIO, the Keras kernel as stored
        conv.__dict__['_mvnerf_packed'] = cached
    return cached[1]


def conv3x3_act(conv, a, b, activation, fused_conv=False, mul=None, amax_a=None, amax_b=None, fused_backward=False):
    """`act(conv([a | b])) * mul` of NCHW a, b (b may be None) with a bias-free 3x3 `conv`; mul (N, C, 1, 1) or None.  Returns (out, amax):
    through torch (amax None) unless `fused_conv` (True | False | 'auto', :func:`_wants_fused`) selects ops.conv3x3, which reads the two
    sources without a concat or a padded copy and returns max |out| as a device float - the next convolution's `amax_a`.  A convolution
    the kernel does not take (:func:`conv3x3_fusable`) runs through torch under 'auto' and raises under True.
    fused_backward: where the call needs a gradient with respect to a or b only - the weight and `mul` frozen - it runs as
    :class:`Conv3x3ActFunction`, HIP in both directions; a weight or `mul` that requires a gradient is not its case: 'auto' uses torch
    and True raises ValueError."""
    if _wants_fused_backward(fused_conv, fused_backward, a, b, conv.weight, mul):
        trains = conv.weight.requires_grad or (mul is not None and mul.requires_grad)
        if trains and fused_conv is True:
            raise ValueError('fused_conv=True with fused_backward: the HIP backward of the fusion covers the data gradient only; freeze '
                             f"the weight and `mul` of this {conv.in_channels} -> {conv.out_channels} convolution or use 'auto'")
        if not trains and conv3x3_fusable(conv, a.shape[1], 0 if b is None else b.shape[1]):
            return Conv3x3ActFunction.apply(a, b, conv.weight, conv, activation, mul, amax_a, amax_b)
        if not trains and fused_conv is True:
            raise ValueError(f'fused_conv=True: a {tuple(conv.kernel_size)} convolution over {a.shape[1]} + {0 if b is None else b.shape[1]} -> '
                             f"{conv.out_channels} channels is not one the HIP pass takes (3x3, no bias, multiples of 32 + 32 -> 64); use 'auto'")
    fused = _wants_fused(fused_conv, a, b, conv.weight, mul, name='fused_conv')
    if fused and not conv3x3_fusable(conv, a.shape[1], 0 if b is None else b.shape[1]):
        if fused_conv is True:
            raise ValueError(f'fused_conv=True: a {tuple(conv.kernel_size)} convolution over {a.shape[1]} + {0 if b is None else b.shape[1]} -> '
                             f"{conv.out_channels} channels is not one the HIP pass takes (3x3, no bias, multiples of 32 + 32 -> 64); use 'auto'")
        fused = False
    if not fused:
        out = _ACT_FNS[activation](conv(a if b is None else torch.cat([a, b], 1)))
        return (out if mul is None else out * mul), None
    from . import ops
    nhwc = lambda t: None if t is None else t.detach().permute(0, 2, 3, 1).contiguous()      # free when the storage is channels-last already
    n, c_out = a.shape[0], conv.out_channels
    if mul is not None:
        mul = mul.detach().reshape(mul.shape[0], c_out).expand(n, c_out).contiguous()
    amax = torch.empty(1, dtype=torch.float32, device=a.device)
    out = ops.conv3x3(nhwc(a), nhwc(b), _packed_conv3x3(conv), c_out, _ACT_CODES[activation], mul=mul, amax_a=amax_a, amax_b=amax_b,
                      amax_out=amax)
    return out.permute(0, 3, 1, 2), amax


CONV3X3_AUTO_MIN_WORKGROUPS = 48


def conv3x3_auto_pays(n, h, w, c_out):
    """The 'auto' rule of the `conv_decode` convolutions, the only ones of VisualFeatures on maps of a few pixels: the kernel's launch has
    n x ceil(h / 16) x ceil(w / 16) x c_out / 64 workgroups, and at the reference's sizes with 3 views it was faster than the torch path in
    every repeat at 48 of them (28 x 28, 96 -> 256) and slower at 12 (14 x 14 and 7 x 7); the figures are the `convs` entries of
    profiles/visual_features_bench.json.  Three shapes at one batch size: the workgroup count as the deciding quantity is
    an extrapolation in n (nothing between 12 and 48 was measured, and with one view the 28 x 28 launch has 16 workgroups and goes to
    torch too) - conservative, since torch is the path that was there before."""
    return n * -(-h // 16) * -(-w // 16) * (c_out // 64) >= CONV3X3_AUTO_MIN_WORKGROUPS


def _fused_or_torch(fused_conv, conv, c_in, *tensors):
    """The switch of one biased convolution of VisualFeatures: :func:`_wants_fused` on the tensors, then the channel counts - a
    convolution the kernel does not take runs through torch under 'auto' and raises under True."""
    fused = _wants_fused(fused_conv, conv.weight, conv.bias, *tensors, name='fused_conv')
    if fused and not conv3x3_fusable(conv, c_in, bias=True):
        if fused_conv is True:
            raise ValueError(f'fused_conv=True: a {tuple(conv.kernel_size)} convolution over {c_in} -> {conv.out_channels} channels is not one '
                             f"the HIP pass takes (3x3, stride 1, multiples of 32 -> 64); use 'auto'")
        fused = False
    return fused


def _nhwc(t):
    return None if t is None else t.detach().permute(0, 2, 3, 1).contiguous()      # free when the storage is channels-last already


def _packed_conv3x3_t(conv):
    """The packed stream of the data gradient's kernel (ops.conv3x3_pack_transposed: `conv.weight` flipped and transposed), cached next
    to :func:`_packed_conv3x3` per parameter version and per load."""
    from . import ops
    weight = conv.weight
    key = (weight._version, weight.data_ptr(), weight.device, conv.__dict__.get('_mvnerf_loads', 0))
    cached = conv.__dict__.get('_mvnerf_packed_t')
    if cached is None or cached[0] != key:
        cached = (key, ops.conv3x3_pack_transposed(weight.detach().permute(2, 3, 1, 0).contiguous()))
        conv.__dict__['_mvnerf_packed_t'] = cached
    return cached[1]


def conv3x3_dgrad_fusable(conv):
    """Whether the data gradient of `conv` is one ops.conv3x3 launch on the transposed pack: its channel counts swap roles, so next to
    the forward's rule the outputs must come in multiples of 32 and the inputs in multiples of 64."""
    return conv.out_channels % 32 == 0 and conv.in_channels % 64 == 0


class Conv3x3BiasFunction(torch.autograd.Function):
    """`conv(act_in(x))` of NCHW x with a 3x3, stride-1 `conv` (bias or none) as HIP passes in both directions.
    forward: the fused launch of :func:`conv3x3_bias`; saves x (NHWC) and its amax.  backward, for g = dL/dout:
      dw, dbias   ops.conv3x3_wgrad of (x, g) with act_in applied as x is staged;
      dx          ops.conv3x3 of g with the flipped, transposed pack (torch.nn.grad.conv2d_input where the channel counts do not fit:
                  :func:`conv3x3_dgrad_fusable`), times act_in'(x) in torch; skipped when x needs no gradient.
    Returns (out NCHW view of NHWC storage, max |out| as a device float)."""

    @staticmethod
    def forward(ctx, x, weight, bias, conv, act_in, amax):
        from . import ops
        xn = _nhwc(x)
        if amax is None:
            amax = ops.absmax(xn)
        top = torch.empty(1, dtype=torch.float32, device=x.device)
        out = ops.conv3x3(xn, None, _packed_conv3x3(conv), conv.out_channels, 0, amax_a=amax, amax_out=top,
                          bias=None if bias is None else bias.detach(), act_in=_ACT_CODES[act_in])
        ctx.save_for_backward(xn, amax, weight)
        ctx.conv, ctx.act_in, ctx.has_bias = conv, act_in, bias is not None
        out = out.permute(0, 3, 1, 2)
        ctx.mark_non_differentiable(top)
        return out, top

    @staticmethod
    def backward(ctx, g, _g_top):
        from . import ops
        xn, amax, weight = ctx.saved_tensors
        conv, act_in = ctx.conv, ctx.act_in
        gn = _nhwc(g)
        amax_g = ops.absmax(gn)
        dx = dw = dbias = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            got = ops.conv3x3_wgrad(xn, gn, _ACT_CODES[act_in], amax_x=amax, amax_g=amax_g, want_bias=ctx.has_bias)
            dw, dbias = got if ctx.has_bias else (got, None)
            dw = dw.permute(3, 2, 0, 1)                              # HWIO -> OIHW
        if ctx.needs_input_grad[0]:
            if conv3x3_dgrad_fusable(conv):
                dx = ops.conv3x3(gn, None, _packed_conv3x3_t(conv), conv.in_channels, 0, amax_a=amax_g).permute(0, 3, 1, 2)
            else:
                dx = torch.nn.grad.conv2d_input((xn.shape[0], xn.shape[3], xn.shape[1], xn.shape[2]), weight.detach(), g, padding=1)
            dx = conv3x3_act_grad(dx, xn.permute(0, 3, 1, 2), act_in)
        return dx, dw, dbias, None, None, None


def conv3x3_act_grad(dx, x, act_in):
    """dx * act_in'(x): relu' = x > 0, elu' = x > 0 ? 1 : exp(x) - an elementwise torch pass on the saved x."""
    if act_in is None:
        return dx
    if act_in == 'relu':
        return dx * (x > 0)
    return dx * torch.where(x > 0, torch.ones_like(x), torch.exp(x))


def _wants_fused_backward(fused_conv, fused_backward, *tensors):
    """The case `fused_backward` is about: a switch that is on (True | 'auto'), everything on the GPU, and a gradient needed - where
    :func:`_wants_fused` says torch ('auto') or raises (True)."""
    if fused_conv is False or not fused_backward:
        return False
    tensors = [t for t in tensors if t is not None]
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors) and all(t.is_cuda for t in tensors)


def _conv3x3_train(conv, x, act_in, fused_conv, amax):
    """The differentiable HIP convolution of a call that needs a gradient -> (out, amax), or None where the kernel does not take the
    convolution under 'auto' (ValueError under True, as in :func:`_fused_or_torch`)."""
    if not conv3x3_fusable(conv, x.shape[1], bias=True):
        if fused_conv is True:
            raise ValueError(f'fused_conv=True: a {tuple(conv.kernel_size)} convolution over {x.shape[1]} -> {conv.out_channels} channels is not '
                             f"one the HIP pass takes (3x3, stride 1, multiples of 32 -> 64); use 'auto'")
        return None
    return Conv3x3BiasFunction.apply(x, conv.weight, conv.bias, conv, act_in, amax)


def conv3x3_bias(conv, x, act_in=None, fused_conv=False, amax=None, fused_backward=False):
    """`conv(act_in(x))` of NCHW x with a biased 3x3 `conv` -> (out, amax | None): through torch unless `fused_conv` selects ops.conv3x3
    with bias and act_in (zero padding after the activation, as torch pads the activated map).  amax bounds |x|; |act_in(x)| <= |x|.
    fused_backward: where the call needs a gradient, :class:`Conv3x3BiasFunction` instead of torch / the "no backward" error."""
    if _wants_fused_backward(fused_conv, fused_backward, conv.weight, conv.bias, x):
        got = _conv3x3_train(conv, x, act_in, fused_conv, amax)
        return got if got is not None else (conv(_ACT_FNS[act_in](x)), None)
    if not _fused_or_torch(fused_conv, conv, x.shape[1], x):
        return conv(_ACT_FNS[act_in](x)), None
    from . import ops
    top = torch.empty(1, dtype=torch.float32, device=x.device)
    out = ops.conv3x3(_nhwc(x), None, _packed_conv3x3(conv), conv.out_channels, 0, amax_a=amax, amax_out=top,
                      bias=None if conv.bias is None else conv.bias.detach(), act_in=_ACT_CODES[act_in])
    return out.permute(0, 3, 1, 2), top


def conv3x3_bn(conv, norm, x, skip=None, fused_conv=False, amax=None, fused_backward=False):
    """`relu(batch_norm(conv(x)) (+ skip))` of NCHW x with a biased 3x3 `conv` and the batch statistics of its own output (gamma, beta,
    eps of `norm`; layers.py:22-33) -> (out, amax | None).  Through torch unless `fused_conv` selects the three HIP passes: ops.conv3x3
    with the bias and the per-tile statistics, ops.bn_finalize, ops.bn_apply in place with the skip, the relu and max |out|.
    fused_backward: where the call needs a gradient, the convolution is :class:`Conv3x3BiasFunction` (no statistics) and the
    normalisation, skip and relu are torch; no apply supplies max |out| then, so the next convolution measures its own input."""
    if _wants_fused_backward(fused_conv, fused_backward, conv.weight, conv.bias, x, skip, norm.weight, norm.bias):
        got = _conv3x3_train(conv, x, None, fused_conv, amax)
        y = got[0] if got is not None else conv(x)
        out = F.batch_norm(y, None, None, norm.weight, norm.bias, True, 0.0, norm.eps)
        return F.relu(out if skip is None else out + skip), None
    if not _fused_or_torch(fused_conv, conv, x.shape[1], x, skip, norm.weight, norm.bias):
        out = F.batch_norm(conv(x), None, None, norm.weight, norm.bias, True, 0.0, norm.eps)
        return F.relu(out if skip is None else out + skip), None
    from . import ops
    n, _, h, w = x.shape
    c_out = conv.out_channels
    y, stats = ops.conv3x3(_nhwc(x), None, _packed_conv3x3(conv), c_out, 0, amax_a=amax,
                           bias=None if conv.bias is None else conv.bias.detach(), stats=True)
    mean, rstd = ops.bn_finalize(stats, n, h, w, c_out, norm.eps)
    top = torch.empty(1, dtype=torch.float32, device=x.device)
    out = ops.bn_apply(y, mean, rstd, norm.weight.detach(), norm.bias.detach(), skip=_nhwc(skip), act='relu', out=y, amax_out=top)
    return out.permute(0, 3, 1, 2), top


def _packed_conv3x3_t_rows(conv, lo, hi):
    """:func:`_packed_conv3x3_t` of the input channels lo:hi of `conv.weight` alone - the data gradient's kernel towards one of the two
    sources of a two-source convolution - cached next to it per parameter version, per load and per slice."""
    from . import ops
    weight = conv.weight
    key = (weight._version, weight.data_ptr(), weight.device, conv.__dict__.get('_mvnerf_loads', 0))
    rows = conv.__dict__.setdefault('_mvnerf_packed_t_rows', {})
    cached = rows.get((lo, hi))
    if cached is None or cached[0] != key:
        cached = (key, ops.conv3x3_pack_transposed(weight.detach()[:, lo:hi].permute(2, 3, 1, 0).contiguous()))
        rows[(lo, hi)] = cached
    return cached[1]


def conv3x3_rows_dgrad_fusable(conv, lo, hi):
    """:func:`conv3x3_dgrad_fusable` on the slice lo:hi of the input channels."""
    return conv.out_channels % 32 == 0 and hi > lo and (hi - lo) % 64 == 0


class Conv3x3ActFunction(torch.autograd.Function):
    """:func:`conv3x3_act` with a FROZEN weight and `mul` as HIP passes in both directions: the gradient of
    out = act(conv([a | b])) * mul with respect to a and b - what the visual features need on their way back through the fusion.
    forward: the ops.conv3x3 launch of the inference path, unchanged; saves `out` (NHWC) and `mul` (N, C) - not a, b or the sum.
    backward, for g = dL/dout:
      d           ops.act_gate(g, out, mul): g * mul * act'(y) from out and mul alone, with max |d| in its amax word (no ops.absmax);
      da          ops.conv3x3 of d with the flipped, transposed pack of the `a` rows of the weight (:func:`_packed_conv3x3_t_rows`),
                  torch.nn.grad.conv2d_input where the slice's channel counts do not fit (:func:`conv3x3_rows_dgrad_fusable`);
      db          the same from the `b` rows, only if b needs a gradient (the CLIP maps never do).
    Returns (out NCHW view of NHWC storage, max |out| as a device float)."""

    @staticmethod
    def forward(ctx, a, b, weight, conv, activation, mul, amax_a, amax_b):
        from . import ops
        an, bn = _nhwc(a), _nhwc(b)
        n, c_out = a.shape[0], conv.out_channels
        if mul is not None:
            mul = mul.detach().reshape(mul.shape[0], c_out).expand(n, c_out).contiguous()
        top = torch.empty(1, dtype=torch.float32, device=a.device)
        out = ops.conv3x3(an, bn, _packed_conv3x3(conv), c_out, _ACT_CODES[activation], mul=mul, amax_a=amax_a, amax_b=amax_b, amax_out=top)
        ctx.save_for_backward(out, mul, weight)
        ctx.conv, ctx.activation, ctx.c_a = conv, activation, a.shape[1]
        ctx.mark_non_differentiable(top)
        return out.permute(0, 3, 1, 2), top

    @staticmethod
    def backward(ctx, g, _g_top):
        from . import ops
        out, mul, weight = ctx.saved_tensors
        conv, c_a = ctx.conv, ctx.c_a
        n, h, w, _ = out.shape
        word = torch.empty(1, dtype=torch.float32, device=out.device)
        d = ops.act_gate(_nhwc(g), out, mul, _ACT_CODES[ctx.activation], amax_out=word)

        def source(lo, hi):
            if conv3x3_rows_dgrad_fusable(conv, lo, hi):
                return ops.conv3x3(d, None, _packed_conv3x3_t_rows(conv, lo, hi), hi - lo, 0, amax_a=word).permute(0, 3, 1, 2)
            return torch.nn.grad.conv2d_input((n, hi - lo, h, w), weight.detach()[:, lo:hi], d.permute(0, 3, 1, 2), padding=1)

        da = source(0, c_a) if ctx.needs_input_grad[0] else None
        db = source(c_a, conv.in_channels) if ctx.needs_input_grad[1] else None
        return da, db, None, None, None, None, None, None


class DoubleConv(nn.Module):
    """layers.py:414-434: two bias-free 3x3 convolutions, the activation after each.
    fused_conv (default False: torch): both as ops.conv3x3 launches, see :func:`conv3x3_act`.
    fused_backward (default False): where a call under `fused_conv` needs a gradient and the weights are frozen, both run as
    :class:`Conv3x3ActFunction`, HIP in both directions."""

    def __init__(self, c_in, filters, activation='relu', fused_conv=False, fused_backward=False):
        super().__init__()
        self.conv_1 = SameConv2d(c_in, filters, 3, bias=False)
        self.conv_2 = SameConv2d(filters, filters, 3, bias=False)
        self.activation = activation
        self.act = _activation(activation)
        self.fused_conv = fused_conv
        self.fused_backward = fused_backward

    @property
    def fused_backward(self):
        return self._fused_backward

    @fused_backward.setter
    def fused_backward(self, value):
        self._fused_backward = _check_bool(value)

    def convs(self, a, b=None, mul=None, amax_a=None, amax_b=None):
        """act(conv_2(act(conv_1([a | b])))) * mul -> (out, amax | None); the first convolution's amax_out is the second one's amax."""
        x, amax = conv3x3_act(self.conv_1, a, b, self.activation, self.fused_conv, None, amax_a, amax_b, self.fused_backward)
        return conv3x3_act(self.conv_2, x, None, self.activation, self.fused_conv, mul, amax, fused_backward=self.fused_backward)

    def forward(self, x):
        if self.fused_conv is False:
            return self.act(self.conv_2(self.act(self.conv_1(x))))
        return self.convs(x)[0]


class Up(nn.Module):
    """layers.py:437-456: [x2 bilinear of x | CLIP stage map resized to `shape`] -> DoubleConv.
    fused_conv (default False: torch): the DoubleConv reads the two maps from where they lie, no concat.
    fused_backward (default False): handed to the DoubleConv."""

    def __init__(self, shape, c_in, c_clip, filters, activation='relu', fused_conv=False, fused_backward=False):
        super().__init__()
        self.shape = tuple(shape)
        self.double_conv = DoubleConv(c_in + c_clip, filters, activation, fused_conv, fused_backward)

    @property
    def fused_backward(self):
        return self.double_conv.fused_backward

    @fused_backward.setter
    def fused_backward(self, value):
        self.double_conv.fused_backward = value

    @property
    def fused_conv(self):
        return self.double_conv.fused_conv

    @fused_conv.setter
    def fused_conv(self, value):
        self.double_conv.fused_conv = value

    def convs(self, x, clip_x, mul=None, amax_x=None):
        """-> (out * mul, amax | None).  amax_x bounds |x|: a bilinear x2 of a map cannot exceed the map's maximum, so it bounds _up(x) too."""
        return self.double_conv.convs(_up(x, 2), _resize(clip_x, self.shape), mul, amax_x)

    def forward(self, x, clip_x):
        if self.fused_conv is False:
            return self.double_conv(torch.cat([_up(x, 2), _resize(clip_x, self.shape)], 1))
        return self.convs(x, clip_x)[0]


class ConvFusion(nn.Module):
    """layers.py:459-477: activation([x1 | x2]) -> bias-free 1x1 convolution (the activation comes BEFORE the convolution)."""

    def __init__(self, c_in, filters, activation='relu'):
        super().__init__()
        self.conv = SameConv2d(c_in, filters, 1, bias=False)
        self.activation = activation
        self.act = _activation(activation)

    def forward(self, x1, x2):
        return self.conv(self.act(torch.cat([x1, x2], 1)))


class Tile(nn.Module):
    """layers.py:494-520: the text embedding through a bias-free Dense (use_dense) or cut to its first `filters` entries (`Slice`),
    as one value per channel; the reference repeats it over `shape`, here it broadcasts."""

    def __init__(self, text_dim=1024, filters=256, use_dense=True):
        super().__init__()
        if not use_dense and filters > text_dim:
            raise ValueError(f'Slice: {filters} filters from a text embedding of {text_dim}')
        self.filters = filters
        self.dense = nn.Linear(text_dim, filters, bias=False) if use_dense else None
        if use_dense:
            nn.init.xavier_uniform_(self.dense.weight)

    def forward(self, clip_textuals):
        x = self.dense(clip_textuals) if self.dense is not None else clip_textuals[:, :self.filters]
        return x[:, :, None, None]


class MultiplyFusion(nn.Module):
    """layers.py:480-491: the feature map times the tiled text embedding, channel by channel."""

    def __init__(self, text_dim=1024, filters=256, use_dense=True):
        super().__init__()
        self.tile = Tile(text_dim, filters, use_dense)

    def forward(self, clip_x, clip_textuals):
        return clip_x * self.tile(clip_textuals)


class CombineCLIPVisualV4(nn.Module):
    """layers.py:593-660 (`LanguageNeRF.combine_clip_visual`, model_v4.py:176-190: use_dense=True, activation='elu'): a U-Net over the
    CLIP stage maps, the text embedding multiplied in at three scales, the visual features fused in at three scales; ends with the
    tail of :class:`CombineCLIPVisualV0` (`conv_fusion_3` + `up_sample`).  up3_filters=128 is V4, 256 is V3 (:523-590), which differs
    in nothing else.  Inputs are NCHW (channels-last storage); the pooled CLIP vector is carried and not used, as in the reference.
    fused_tail: 'auto' | True | False - the tail as one HIP pass (:func:`conv_fusion_tail`) when on the GPU and nothing needs a gradient.
    fused_backward: False (default) | True - where a call under `fused_tail` needs a gradient and the output is fp32, the tail runs as
    :class:`FuseUpsample2xFunction`, HIP in both directions; it is also handed to `up_1..3`, whose convolutions under `fused_conv` then
    run as :class:`Conv3x3ActFunction` where a gradient flows to the visual features and the fusion's weights are frozen.
    fused_conv: False (default) | True | 'auto' - the seven 3x3 convolutions as ops.conv3x3 launches under the same rule
    (:func:`conv3x3_act`), `multiply_fusion_1..3` in the epilogue of the convolution in front of them, every amax_out the next amax.
    Parity unpinned, like the rest of this file."""

    def __init__(self, use_dense=False, activation='relu', half_size=(240, 320), clip_channels=(256, 512, 1024, 2048), text_dim=1024,
                 widths=(1024, 512, 256), up3_filters=128, visual_channels=256, filters=256, fused_tail='auto', fused_conv=False,
                 fused_backward=False):
        super().__init__()
        hh, hw = half_size
        if hh % 8 or hw % 8:
            raise ValueError(f'half size {half_size}: both must be multiples of 8 (three x2 up-samplings end there)')
        c1, c2, c3, c4 = clip_channels
        w1, w2, w3 = widths
        self.half_size = (hh, hw)
        self.text_dim = text_dim
        self.size_1,self.size_2, self.size_3 = (hh // 2, hw // 2), (hh // 4, hw // 4), (hh // 8, hw // 8)
        self.activation = activation
        self.act = _activation(activation)
        self.conv = SameConv2d(c4, w1, 3, bias=False)                                   # Conv2D(..., activation=activation)
        self.multiply_fusion_1 = MultiplyFusion(text_dim, w1, use_dense)
        self.up_1 = Up(self.size_2, w1, c3, w2, activation)
        self.multiply_fusion_2 = MultiplyFusion(text_dim, w2, use_dense)
        self.conv_fusion_1 = ConvFusion(w2 + visual_channels, w2, activation)
        self.up_2 = Up(self.size_1, w2, c2, w3, activation)
        self.multiply_fusion_3 = MultiplyFusion(text_dim, w3, use_dense)
        self.conv_fusion_2 = ConvFusion(w3 + visual_channels, w3, activation)
        self.up_3 = Up(self.half_size, w3, c1, up3_filters, activation)
        self.conv_fusion_3 = ConvFusion(up3_filters + visual_channels, filters, activation)
        self.fused_tail = fused_tail
        self.fused_conv = fused_conv
        self.fused_backward = fused_backward

    @property
    def fused_backward(self):
        return self._fused_backward

    @fused_backward.setter
    def fused_backward(self, value):
        self._fused_backward = _check_bool(value)
        for up in (self.up_1, self.up_2, self.up_3):
            up.fused_backward = value

    @property
    def fused_conv(self):
        return self._fused_conv

    @fused_conv.setter
    def fused_conv(self, value):
        if value not in (True, False, 'auto'):
            raise ValueError(f"fused_conv: {value!r}, expected True, False or 'auto'")
        self._fused_conv = value
        for up in (self.up_1, self.up_2, self.up_3):
            up.fused_conv = value

    def forward(self, clip_outputs, visual_features, clip_textuals, out_dtype=None):
        _clip_visuals, clip_l1, clip_l2, clip_l3, clip_l4 = clip_outputs
        vis_1 = _resize(visual_features, self.size_1)
        vis_2 = _resize(visual_features, self.size_2)
        if self.fused_conv is False:
            x = self.act(self.conv(_resize(clip_l4, self.size_3)))
            x = self.multiply_fusion_1(x, clip_textuals)
            x = self.up_1(x, clip_l3)
            x = self.multiply_fusion_2(x, clip_textuals)
            x = self.conv_fusion_1(x, vis_2)
            x = self.up_2(x, clip_l2)
            x = self.multiply_fusion_3(x, clip_textuals)
            x = self.conv_fusion_2(x, vis_1)
            x = self.up_3(x, clip_l1)
        else:               # the same chain; each MultiplyFusion is the `mul` of the convolution in front of it
            tile = lambda fusion: fusion.tile(clip_textuals)
            x, amax = conv3x3_act(self.conv, _resize(clip_l4, self.size_3), None, self.activation, self.fused_conv, tile(self.multiply_fusion_1),
                                  fused_backward=self.fused_backward)
            x, _ = self.up_1.convs(x, clip_l3, tile(self.multiply_fusion_2), amax)
            x = self.conv_fusion_1(x, vis_2)
            x, _ = self.up_2.convs(x, clip_l2, tile(self.multiply_fusion_3))
            x = self.conv_fusion_2(x, vis_1)
            x, _ = self.up_3.convs(x, clip_l1)
        fused = _tail_switch(self.fused_tail, self.fused_backward and out_dtype in (None, torch.float32), x, visual_features,
                             self.conv_fusion_3.conv.weight)
        return conv_fusion_tail(x, visual_features, self.conv_fusion_3.conv, self.activation, fused, out_dtype)


# ---- stand-ins for CLIP (its RN50 trunk, text transformer and BPE vocabulary are not available offline) ------------------------------
class SyntheticCLIPPyramid(nn.Module):
    """Frozen, seeded stand-in for the CLIP RN50 visual trunk with its stage outputs (clip/model.py): images (N, 3, H, W) ->
    (pooled (N, embed_dim), stage maps (N, c_i, s_i, s_i) for the four stages).  Not trained, carries no semantics."""

    def __init__(self, channels=(256, 512, 1024, 2048), sizes=(56, 28, 14, 7), embed_dim=1024, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.register_buffer('w_stem', torch.randn(channels[0], 3, 7, 7, generator=g) * 0.1)
        for i in range(1, 4):
            self.register_buffer(f'w_{i}', torch.randn(channels[i], channels[i - 1], 1, 1, generator=g) * (2.0 / channels[i - 1]) ** 0.5)
        self.register_buffer('w_pool', torch.randn(embed_dim, channels[3], generator=g) * (1.0 / channels[3]) ** 0.5)
        self.sizes = tuple((s, s) if isinstance(s, int) else tuple(s) for s in sizes)

    @torch.no_grad()
    def forward(self, x_nchw):
        maps = [F.relu(F.adaptive_avg_pool2d(F.conv2d(x_nchw, self.w_stem, stride=2, padding=3), self.sizes[0]))]
        for i in range(1, 4):
            maps.append(F.relu(F.conv2d(F.adaptive_avg_pool2d(maps[-1], self.sizes[i]), getattr(self, f'w_{i}'))))
        pooled = F.linear(maps[-1].mean((2, 3)), self.w_pool)
        return (pooled, *maps)


class SyntheticCLIPText(nn.Module):
    """Frozen, seeded stand-in for CLIP's text transformer: token ids (N, 77) int32 (0 = padding) -> (N, embed_dim).  A token
    table times a position table, summed over the instruction and scaled to unit RMS: different instructions give different
    embeddings, word order counts, nothing is learnt."""

    def __init__(self, vocab_size=49408, embed_dim=1024, context_length=77, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.register_buffer('token_table', torch.randn(vocab_size, embed_dim, generator=g))
        self.register_buffer('position_table', 1.0 + 0.5 * torch.randn(context_length, embed_dim, generator=g))

    @torch.no_grad()
    def forward(self, tokens):
        tokens = torch.as_tensor(tokens, device=self.token_table.device).long()
        if tokens.dim() != 2 or tokens.shape[1] != self.position_table.shape[0]:
            raise ValueError(f'tokens: shape {tuple(tokens.shape)}, expected (N, {self.position_table.shape[0]})')
        mask = (tokens != 0).to(self.token_table.dtype)[..., None]
        e = (self.token_table[tokens % self.token_table.shape[0]] * self.position_table * mask).sum(1)
        return e / e.pow(2).mean(1, keepdim=True).sqrt().clamp_min(1e-6)


def tokenize(texts, context_length=77):
    """The shape and dtype of the reference's `clip/utils.tokenize`: str or list of str -> int32 (N, context_length), zero padded.
    The ids are NOT CLIP's (its BPE vocabulary is not available offline): words and punctuation marks, lower-cased, get the id
    1 + crc32(word) mod 49 405, between a start (49 406) and an end (49 407) id as CLIP places them.  Deterministic across runs."""
    import re
    import zlib
    if isinstance(texts, str):
        texts = [texts]
    out = np.zeros((len(texts), context_length), dtype=np.int32)
    for n, text in enumerate(texts):
        words = re.findall(r'[a-z0-9]+|[^\sa-z0-9]', text.lower())
        ids = [49406] + [1 + zlib.crc32(word.encode('utf-8')) % 49405 for word in words] + [49407]
        if len(ids) > context_length:
            raise RuntimeError(f'Input {text!r} is too long for context length {context_length}')
        out[n, :len(ids)] = ids
    return out


class LanguageFeatureProducer(nn.Module):
    """`LanguageNeRF`'s encoder prologue (model_v4.py:176-190, 277-288) as one frozen callable: images (N, H, W, 3) in [0, 1] and an
    instruction - `tokens` (N | 1, 77) int32 through the text stand-in, or a ready `text_embedding` (N | 1, text_dim) - ->
    combined_features (N, H, W, 256), NHWC-contiguous in `out_dtype`.  VisualFeatures + the CLIP pyramid + the text embedding +
    CombineCLIPVisualV4(use_dense=True, activation='elu').  Nothing in it trains (the reference's tape watches `grasp_readout` only),
    so with fused_tail='auto' the tail is the fused HIP pass whenever the producer is on the GPU; fused_conv (default False) is handed
    to the fusion: its 3x3 convolutions as ops.conv3x3 launches; fused_visual (default False) is the `fused_conv` of VisualFeatures,
    fused_vit (default False) its `fused_vit`: the ViT's transformer blocks as HIP launches."""

    def __init__(self, original_image_size=(480, 640), out_dtype=torch.float32, fused_tail='auto', n_features=256, clip_pyramid=None,
                 clip_text=None, combine_kw=None, fused_conv=False, fused_visual=False, fused_vit=False, **visual_kw):
        super().__init__()
        h, w = original_image_size
        if h % 16 or w % 16:
            raise ValueError('image height and width must be multiples of 16 (the fusion starts at 1/16 resolution)')
        self.visual_features = VisualFeatures(n_features, original_image_size, fused_conv=fused_visual, fused_vit=fused_vit, **visual_kw)
        self.clip_pyramid = clip_pyramid if clip_pyramid is not None else SyntheticCLIPPyramid()
        self.clip_text = clip_text if clip_text is not None else SyntheticCLIPText()
        kw = dict(use_dense=True, activation='elu', half_size=(h // 2, w // 2), visual_channels=n_features, fused_tail=fused_tail,
                  fused_conv=fused_conv)
        kw.update(combine_kw or {})
        self.combine_clip_visual = CombineCLIPVisualV4(**kw)
        self.out_dtype = out_dtype
        self.requires_grad_(False)
        self.eval()

    def train(self, mode=True):
        return super().train(False)                                    # frozen: stays in inference mode

    @torch.no_grad()
    def forward(self, images_nhwc, tokens=None, text_embedding=None):
        if (tokens is None) == (text_embedding is None):
            raise ValueError('give exactly one of tokens (N, 77) and text_embedding (N, text_dim)')
        text = self.clip_text(tokens) if text_embedding is None else text_embedding
        text = text.to(images_nhwc.dtype).expand(images_nhwc.shape[0], -1)
        visual = self.visual_features(images_nhwc)
        pyramid = self.clip_pyramid(images_nhwc.permute(0, 3, 1, 2))
        fused = self.combine_clip_visual(pyramid, visual, text, out_dtype=self.out_dtype)      # (N, 256, H, W), channels-last storage
        out = fused.permute(0, 2, 3, 1).to(self.out_dtype)
        return out if out.is_contiguous() else out.contiguous()


class FeatureProducerV4(nn.Module):
    """The V4 renderer's encoder prologue (mvnerf/model_v4.py:31, 82-84, 196-240) as one callable: images (N, H, W, 3) in [0, 1] ->
    combined_features (N, H, W, 256), NHWC-contiguous in `out_dtype`, through VisualFeatures, the CLIP pyramid and
    CombineCLIPVisualV4(use_dense=False, activation='relu') - the renderer's settings; `LanguageNeRF` builds the same fusion with
    True / 'elu', so both are arguments - with a constant all-ones text embedding unless one is given.  Use it as
    `MVVNeRFRenderer(feature_encoder=producer)`: the renderer trains `visual_features` THROUGH the language fusion and writes the
    sub-model files `LanguageNeRF.load_backbone` reads.  `trainable_parameters()` is :class:`FeatureProducer`'s list (vision_transformer
    + conv_features); the fusion and the pyramid are frozen (`requires_grad_(False)`), the pyramid runs under `no_grad`.
    fused_tail / fused_conv / fused_backward are the fusion's switches, fused_visual the `fused_conv` of VisualFeatures (which gets
    `fused_backward` too), everything else (`fused_vit`, the ViT's sizes) goes to VisualFeatures."""

    def __init__(self, original_image_size=(480, 640), n_features=256, clip_pyramid=None, out_dtype=torch.float32, use_dense=False,
                 activation='relu', fused_tail='auto', fused_conv=False, fused_backward=False, fused_visual=False, combine_kw=None,
                 **visual_kw):
        super().__init__()
        h, w = original_image_size
        if h % 16 or w % 16:
            raise ValueError('image height and width must be multiples of 16 (the fusion starts at 1/16 resolution)')
        self.visual_features = VisualFeatures(n_features, original_image_size, fused_conv=fused_visual, fused_backward=fused_backward,
                                              **visual_kw)
        self.clip_pyramid = clip_pyramid if clip_pyramid is not None else SyntheticCLIPPyramid()
        kw = dict(use_dense=use_dense, activation=activation, half_size=(h // 2, w // 2), visual_channels=n_features, fused_tail=fused_tail,
                  fused_conv=fused_conv, fused_backward=fused_backward)
        kw.update(combine_kw or {})
        self.combine_clip_visual = CombineCLIPVisualV4(**kw)
        self.text_dim = self.combine_clip_visual.text_dim
        self.out_dtype = out_dtype
        self.combine_clip_visual.requires_grad_(False)
        self.clip_pyramid.requires_grad_(False)

    def trainable_parameters(self):
        return list(self.visual_features.vision_transformer.parameters()) + list(self.visual_features.conv_features.parameters())

    def forward(self, images_nhwc, text_embedding=None):
        n = images_nhwc.shape[0]
        if text_embedding is None:
            text = torch.ones(n, self.text_dim, dtype=images_nhwc.dtype, device=images_nhwc.device)       # model_v4.py:31
        else:
            text = text_embedding.to(images_nhwc.dtype).expand(n, -1)
        visual = self.visual_features(images_nhwc)
        with torch.no_grad():
            pyramid = self.clip_pyramid(images_nhwc.permute(0, 3, 1, 2))
        fused = self.combine_clip_visual(pyramid, visual, text, out_dtype=self.out_dtype)      # (N, 256, H, W), channels-last storage
        out = fused.permute(0, 2, 3, 1).to(self.out_dtype)
        return out if out.is_contiguous() else out.contiguous()


COMBINE_CLIP_VISUAL_V4_VARIABLES = ('conv', 'multiply_fusion_1.tile.dense', 'up_1.double_conv.conv_1', 'up_1.double_conv.conv_2',
                                    'multiply_fusion_2.tile.dense', 'conv_fusion_1.conv', 'up_2.double_conv.conv_1',
                                    'up_2.double_conv.conv_2', 'multiply_fusion_3.tile.dense', 'conv_fusion_2.conv',
                                    'up_3.double_conv.conv_1', 'up_3.double_conv.conv_2', 'conv_fusion_3.conv')


def load_combine_clip_visual_v4(module, arrays):
    """`CombineCLIPVisualV4.weights` (Keras lists a model's variables in the order `__init__` assigns its layers, layers.py:597-618)
    as plain arrays -> `module`, in place: COMBINE_CLIP_VISUAL_V4_VARIABLES, i.e. 13 kernels with use_dense=True (36 814 848 floats at
    the reference's sizes) and the 10 non-Dense ones with use_dense=False (`Slice` has no variable).  Conv2D kernels are (kh, kw, in,
    out), Dense kernels (in, out).  A shape mismatch raises and names the variable.  PARITY UNPINNED: the order could not be checked
    against a TensorFlow dump here."""
    names = [n for n in COMBINE_CLIP_VISUAL_V4_VARIABLES if module.multiply_fusion_1.tile.dense is not None or not n.endswith('.dense')]
    arrays = list(arrays)
    if len(arrays) != len(names):
        raise ValueError(f'combine_clip_visual: {len(arrays)} variables, expected {len(names)}: {names}')
    with torch.no_grad():
        for name, array in zip(names, arrays):
            layer = module.get_submodule(name)
            array = np.asarray(array)
            is_dense = isinstance(layer, nn.Linear)
            expected = ((layer.in_features, layer.out_features) if is_dense else
                        (*layer.kernel_size, layer.in_channels, layer.out_channels))
            if tuple(array.shape) != expected:
                raise ValueError(f'combine_clip_visual: variable {name!r} has shape {tuple(array.shape)}, expected {expected}')
            t = torch.as_tensor(array).to(layer.weight.dtype)
            layer.weight.copy_(t.T if is_dense else t.permute(3, 2, 0, 1))


# ---- Keras variables -> this package (plain arrays; no TensorFlow needed) ------------------------------------------------
# The reference stores one TensorFlow checkpoint per sub-model (model_v0.py:199-214).  Dump each in the reference's own
# environment with, e.g.,
#     r = tf.train.load_checkpoint(f'{path}_coarse_embedding'); np.savez(out, **{k: r.get_tensor(k) for k, _ in tf.train.list_variables(...)})
# or simply `np.savez(out, *[w.numpy() for w in model.coarse_embedding.weights])` - the functions below take the arrays in
# `layer.weights` order (Keras creation order), which for these sub-models is:
#   *_embedding (MVResNetMLPNeRFEmbedding, layers.py:334-379): Dense0 kernel (379,128), bias (128); then per ResNetMLPBlock
#       (6 of them, :262-298): dense_1 kernel (128,128), bias, dense_2 kernel (128,128), bias            -> 246 784 floats
#   *_readout (RenderReadout, :382-397): Dense kernel (128,4), bias (4)                                   ->     516 floats
# which is exactly the flat Keras-order buffer `MVVNeRFRenderer.set_weights` takes (kernel[in,out] row-major, then bias).

MLP_EMBEDDING_SHAPES = [(379, 128), (128,)] + [s for _ in range(6) for s in ((128, 128), (128,), (128, 128), (128,))]
MLP_READOUT_SHAPES = [(128, 4), (4,)]


def flat_net_from_keras(embedding_weights, readout_weights):
    """`[w.numpy() for w in embedding.weights]`, `[... readout.weights]` -> the 247 300-float buffer of one MLP."""
    parts = []
    for arrays, shapes, what in ((embedding_weights, MLP_EMBEDDING_SHAPES, 'embedding'), (readout_weights, MLP_READOUT_SHAPES, 'readout')):
        arrays = [np.asarray(a, dtype=np.float32) for a in arrays]
        if [a.shape for a in arrays] != shapes:
            raise ValueError(f'{what}: variable shapes {[a.shape for a in arrays]} do not match the Keras creation order {shapes}')
        parts += [a.reshape(-1) for a in arrays]
    flat = np.concatenate(parts)
    assert flat.size == 247300
    return flat


def keras_from_flat_net(flat):
    """Inverse of :func:`flat_net_from_keras`: (embedding arrays, readout arrays) for `layer.set_weights`."""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    out, pos = [], 0
    for shape in MLP_EMBEDDING_SHAPES + MLP_READOUT_SHAPES:
        n = int(np.prod(shape))
        out.append(flat[pos:pos + n].reshape(shape).copy())
        pos += n
    return out[:len(MLP_EMBEDDING_SHAPES)], out[len(MLP_EMBEDDING_SHAPES):]


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32))


def load_conv(conv, kernel_hwio, bias=None):
    """Keras Conv2D kernel (kh, kw, in, out) -> torch (out, in, kh, kw)."""
    conv.weight.data.copy_(_t(kernel_hwio).permute(3, 2, 0, 1))
    conv.__dict__.pop('_mvnerf_packed', None)            # (`.data` does not bump the parameter version the packed-stream cache keys on)
    conv.__dict__.pop('_mvnerf_packed_t', None)
    conv.__dict__.pop('_mvnerf_packed_t_rows', None)
    if bias is not None:
        conv.bias.data.copy_(_t(bias))


def load_conv_transpose(conv, kernel_hwoi, bias):
    """Keras Conv2DTranspose kernel (kh, kw, out, in) -> torch ConvTranspose2d (in, out, kh, kw)."""
    conv.weight.data.copy_(_t(kernel_hwoi).permute(3, 2, 0, 1))
    conv.bias.data.copy_(_t(bias))


def load_dense(lin, kernel_io, bias):
    """Keras Dense kernel (in, out) -> torch Linear (out, in)."""
    lin.weight.data.copy_(_t(kernel_io).T)
    lin.bias.data.copy_(_t(bias))
    _mark_loaded(lin)                                    # (the packed-stream caches of the fused transformer block)


def load_grasp_readout(readout, arrays):
    """delta_ngf/layers.py:8-42 `GraspReadout.weights` (Keras creation order) -> `lmvnerf.GraspReadout`, copied in place:
    activation_downscale_1..4 (kernel (128,64), bias each); combined_activation_downscale (kernel (256,64), bias); the `readout`
    Sequential: ResNetMLPBlock (layer_0 kernel, bias; layer_1 kernel, bias; shortcut kernel, no bias; mvnerf/layers.py:262-298),
    ResNetMLPBlock (layer_0, layer_1), Readout(1) (output_layer kernel, bias when the module has one)."""
    dense = [(lin, True) for lin in (*readout.activation_downscale, readout.combined_activation_downscale)]
    dense += [(readout.block_0.layer_0, True), (readout.block_0.layer_1, True), (readout.block_0.shortcut, False),
              (readout.block_1.layer_0, True), (readout.block_1.layer_1, True),
              (readout.output_layer, readout.output_layer.bias is not None)]
    expected = []
    for lin, has_bias in dense:
        expected += [(lin.in_features, lin.out_features)] + ([(lin.out_features,)] if has_bias else [])
    arrays = [np.asarray(a, dtype=np.float32) for a in arrays]
    if [a.shape for a in arrays] != expected:
        raise ValueError(f'grasp readout: variable shapes {[a.shape for a in arrays]} do not match the Keras creation order {expected}')
    it = iter(arrays)
    with torch.no_grad():
        for lin, has_bias in dense:
            lin.weight.copy_(_t(next(it)).T)
            if has_bias:
                lin.bias.copy_(_t(next(it)))


def load_batchnorm(bn, gamma, beta, moving_mean, moving_var):
    bn.weight.data.copy_(_t(gamma))
    bn.bias.data.copy_(_t(beta))
    bn.running_mean.data.copy_(_t(moving_mean))
    bn.running_var.data.copy_(_t(moving_var))
    _mark_loaded(bn)


def load_mha(mha, q_k, q_b, k_k, k_b, v_k, v_b, o_k, o_b):
    """Keras MultiHeadAttention: query/key/value kernels (embed, heads, dim) + biases (heads, dim); output kernel (heads, dim, embed)."""
    for lin, k, b in ((mha.q, q_k, q_b), (mha.k, k_k, k_b), (mha.v, v_k, v_b)):
        k = np.asarray(k, dtype=np.float32)
        load_dense(lin, k.reshape(k.shape[0], -1), np.asarray(b).reshape(-1))
    o_k = np.asarray(o_k, dtype=np.float32)
    load_dense(mha.o, o_k.reshape(-1, o_k.shape[-1]), o_b)
    _mark_loaded(mha)


def load_combine_clip_visual(module, weights):
    """CombineCLIPVisualV0.weights = [conv kernel (1, 1, 512, 256)]."""
    (kernel,) = weights
    load_conv(module.conv, kernel)


def load_convolutional_encoder(enc, weights, order='keras'):
    """ConvolutionalEncoder variables (layers.py:36-57) as plain arrays.

    order='keras' (default): the order of Keras' `ConvolutionalEncoder.weights`, i.e. `[w.numpy() for w in enc.weights]`: a
    container lists the weights of its sub-layers in attribute-creation order, and a plain `Layer` (the reference's `Block`)
    lists ALL its trainable variables first and its non-trainable ones (the BatchNormalization moving statistics) after them:
      Sequential: stem conv kernel; stem BN gamma, beta, moving_mean, moving_var;
      Block 1 (has the downsample branch): conv_1 kernel, bias; conv_2 kernel, bias; norm_1 gamma, beta; downsample conv kernel;
                                           downsample BN gamma, beta | norm_1 moving_mean, moving_var; downsample BN moving_mean, moving_var;
      Blocks 2, 3: conv_1 kernel, bias; conv_2 kernel, bias; norm_1 gamma, beta | norm_1 moving_mean, moving_var.
    order='creation' (round 2's reading): downsample conv kernel, downsample BN (gamma, beta, mean, var); stem conv kernel, stem BN (4);
    per Block conv_1 kernel, bias, conv_2 kernel, bias, norm_1 (gamma, beta, mean, var).
    Neither order could be checked against a TensorFlow dump here (no TF, no checkpoint in the reference): PARITY UNPINNED.  Prefer
    keying by variable name (tf.train.list_variables) when a real checkpoint is at hand; a wrong order fails on a shape mismatch
    for the stem / downsample variables but NOT between same-shaped Block variables."""
    w = list(weights)
    seq = enc.conv_features
    blocks = (seq[3], seq[4], seq[5])
    down = seq[3].downsample
    if order == 'creation':
        load_conv(down[0], w.pop(0))
        load_batchnorm(down[1], *[w.pop(0) for _ in range(4)])
        load_conv(seq[0], w.pop(0))
        load_batchnorm(seq[1], *[w.pop(0) for _ in range(4)])
        for blk in blocks:
            load_conv(blk.conv_1, w.pop(0), w.pop(0))
            load_conv(blk.conv_2, w.pop(0), w.pop(0))
            load_batchnorm(blk.norm_1, *[w.pop(0) for _ in range(4)])
    elif order == 'keras':
        load_conv(seq[0], w.pop(0))
        load_batchnorm(seq[1], *[w.pop(0) for _ in range(4)])
        for i, blk in enumerate(blocks):
            load_conv(blk.conv_1, w.pop(0), w.pop(0))
            load_conv(blk.conv_2, w.pop(0), w.pop(0))
            gamma, beta = w.pop(0), w.pop(0)
            if i == 0:
                load_conv(down[0], w.pop(0))
                d_gamma, d_beta = w.pop(0), w.pop(0)
            mean, var = w.pop(0), w.pop(0)
            load_batchnorm(blk.norm_1, gamma, beta, mean, var)
            if i == 0:
                load_batchnorm(down[1], d_gamma, d_beta, w.pop(0), w.pop(0))
    else:
        raise ValueError(f"order: {order!r}, expected 'keras' or 'creation'")
    if w:
        raise ValueError(f'{len(w)} unused variables')


def convolutional_encoder_weights(enc, order='keras'):
    """The inverse of load_convolutional_encoder: this module's variables as Keras-layout arrays in the same order."""
    k_conv = lambda c: c.weight.detach().permute(2, 3, 1, 0).cpu().numpy()
    bn4 = lambda b: [b.weight.detach().cpu().numpy(), b.bias.detach().cpu().numpy(), b.running_mean.cpu().numpy(), b.running_var.cpu().numpy()]
    seq = enc.conv_features
    blocks = (seq[3], seq[4], seq[5])
    down = seq[3].downsample
    out = []
    if order == 'creation':
        out += [k_conv(down[0])] + bn4(down[1]) + [k_conv(seq[0])] + bn4(seq[1])
        for blk in blocks:
            out += [k_conv(blk.conv_1), blk.conv_1.bias.detach().cpu().numpy(), k_conv(blk.conv_2), blk.conv_2.bias.detach().cpu().numpy()] + bn4(blk.norm_1)
        return out
    out += [k_conv(seq[0])] + bn4(seq[1])
    for i, blk in enumerate(blocks):
        out += [k_conv(blk.conv_1), blk.conv_1.bias.detach().cpu().numpy(), k_conv(blk.conv_2), blk.conv_2.bias.detach().cpu().numpy()]
        n = bn4(blk.norm_1)
        out += n[:2]
        if i == 0:
            d = bn4(down[1])
            out += [k_conv(down[0])] + d[:2]
        out += n[2:]
        if i == 0:
            out += d[2:]
    return out


def load_transformer_block(blk, weights):
    """TransformerBlock.weights (layers.py:73-86): BN (gamma, beta, mean, var), MHA (q k, q b, k k, k b, v k, v b, out k, out b),
    LayerNorm (gamma, beta), dense_0 (kernel, bias), dense_1 (kernel, bias)."""
    w = list(weights)
    load_batchnorm(blk.layer_norm_1, *[w.pop(0) for _ in range(4)])
    load_mha(blk.attention, *[w.pop(0) for _ in range(8)])
    blk.layer_norm_2.weight.data.copy_(_t(w.pop(0)))
    blk.layer_norm_2.bias.data.copy_(_t(w.pop(0)))
    load_dense(blk.dense_0, w.pop(0), w.pop(0))
    load_dense(blk.dense_1, w.pop(0), w.pop(0))
    if w:
        raise ValueError(f'{len(w)} unused variables')


def warmup_lr_lambda(warmup_steps=10000, scale_down_after=450000):
    """`torch.optim.lr_scheduler.LambdaLR` factor of nerf_utils.WarmupScheduler (nerf_utils.py:288-300) relative to the target
    rate: the reference's feature optimizer is Adam(WarmupScheduler(1e-5, 10000, 450000)) (train_nerf.py:24-26)."""
    warm = max(1.0, float(warmup_steps))

    def factor(step):
        if step <= warm:
            return step / warm
        return 1.0 if step <= scale_down_after else 0.1
    return factor


class KerasAdam(torch.optim.Optimizer):
    """tf.keras.optimizers.Adam's update (the reference's optimizer_feature, train_nerf.py:24-26), which is NOT torch.optim.Adam's:
        lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t);   p -= lr_t * m / (sqrt(v) + eps)
    torch adds eps to sqrt(v_hat) after the bias correction, i.e. an effective epsilon larger by 1 / sqrt(1 - beta2^t) (31x at t = 1).
    The MLP group of the same train_step (mvnerf_adam_clip) uses the Keras form too."""

    def __init__(self, params, lr=1e-5, betas=(0.9, 0.999), eps=1e-7):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            b1, b2 = group['betas']
            for p in group['params']:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st['step'] = 0
                    st['m'] = torch.zeros_like(p)
                    st['v'] = torch.zeros_like(p)
                st['step'] += 1
                t = st['step']
                st['m'].mul_(b1).add_(p.grad, alpha=1.0 - b1)
                st['v'].mul_(b2).addcmul_(p.grad, p.grad, value=1.0 - b2)
                lr_t = group['lr'] * (1.0 - b2 ** t) ** 0.5 / (1.0 - b1 ** t)
                p.addcdiv_(st['m'], st['v'].sqrt().add_(group['eps']), value=-lr_t)
        return loss


def make_encoder_optimizer(producer, target_lr=1e-5, warmup_steps=10000, scale_down_after=450000):
    """The reference's `optimizer_feature` (train_nerf.py:24-31): Keras Adam (eps 1e-7, Keras' update form: KerasAdam above) on
    vision_transformer + conv_features with the warm-up schedule.  Returns (optimizer, scheduler); call `scheduler.step()` after every
    `train_step`."""
    opt = KerasAdam(producer.trainable_parameters(), lr=target_lr, betas=(0.9, 0.999), eps=1e-7)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, warmup_lr_lambda(warmup_steps, scale_down_after))
    return opt, sched


def count_parameters(module):
    return sum(p.numel() for p in module.parameters())


__all__ = ['FeatureProducer', 'FeatureProducerV4', 'Conv3x3ActFunction', 'LanguageFeatureProducer', 'CombineCLIPVisualV4', 'DoubleConv', 'Up', 'ConvFusion', 'Tile',
           'MultiplyFusion', 'conv3x3_act', 'conv3x3_bias', 'conv3x3_bn', 'conv3x3_auto_pays', 'conv3x3_fusable', 'Block', 'SyntheticCLIPPyramid', 'SyntheticCLIPText', 'tokenize', 'conv_fusion_tail', 'load_combine_clip_visual_v4',
           'COMBINE_CLIP_VISUAL_V4_VARIABLES', 'VisualFeatures', 'CombineCLIPVisualV0', 'ConvolutionalEncoder', 'VisionTransformerEncoder',
           'VisionTransformer', 'TransformerBlock', 'transformer_block_fused', 'vit_block_unfusable', 'SyntheticCLIPStage1', 'flat_net_from_keras', 'keras_from_flat_net',
           'make_encoder_optimizer', 'KerasAdam', 'convolutional_encoder_weights', 'warmup_lr_lambda', 'load_conv', 'load_conv_transpose', 'load_dense', 'load_batchnorm', 'load_mha',
           'load_combine_clip_visual', 'load_grasp_readout', 'load_convolutional_encoder', 'load_transformer_block', 'count_parameters']
