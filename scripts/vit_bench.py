"""The ViT's transformer blocks as HIP passes (encoders.py `fused_vit`; csrc/token_linear.hip, csrc/attention.hip) against the torch
path, on the GPU (fails without one):

    python scripts/vit_bench.py [--out profiles/vit_bench.json] [--skip-producer]

At 3 views, the reference's sizes (3 x 197 tokens of 768 channels, 12 heads of 64): the four Dense shapes at M = 591 against F.linear
(+ gelu / + residual), attention against F.scaled_dot_product_attention, LayerNorm (each with an amax word zeroed once, as the block
zeroes its four words in one fill), one TransformerBlock, the 12-block VisionTransformer, then VisualFeatures alone and the whole
LanguageFeatureProducer per view with and without the switch, and one run under forward hooks for the per-stage split of
VisualFeatures.  Single passes and modules up to the ViT run with fused_vit=True (every pass in HIP); VisualFeatures with 'auto' (the
setting a user would pick: encoders.VIT_AUTO_TORCH_PASSES routes single passes back to torch) and with True, the producer with 'auto'.
All modules are in eval mode, which the fused block needs.  Both paths run in this process, every case warmed up, alternating windows
of at least 0.5 s timed with device events, three repeats (median, min - max)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.visual_features_bench import alternate, stage_split  # noqa: E402
from thesis_clip_nerf_amd import encoders as E  # noqa: E402
from thesis_clip_nerf_amd import ops  # noqa: E402

TOKENS, EMBED, HEADS = 197, 768, 12
# name, K, N, epilogue
DENSE_SHAPES = [('qkv', 768, 2304, None), ('out_projection', 768, 768, 'residual'), ('dense_0', 768, 3072, 'gelu'),
                ('dense_1', 3072, 768, 'residual')]


def dense_case(name, m, k, n, epi, repeats):
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(m, k, device='cuda', generator=g)
    w = (torch.rand(n, k, device='cuda', generator=g) * 2 - 1) * (6.0 / (k + n)) ** 0.5
    bias = 0.2 * torch.randn(n, device='cuda', generator=g)
    res = torch.randn(m, n, device='cuda', generator=g) if epi == 'residual' else None
    packed, amax = ops.linear_pack(w), ops.absmax(x)                          # in the block amax is the previous pass's amax_out
    top = torch.zeros(1, device='cuda')                                       # zeroed once, as the block zeroes its four words in one fill
    fused = lambda: ops.linear(x, packed, n, bias=bias, act='gelu' if epi == 'gelu' else None, residual=res, amax_x=amax, amax_out=top,
                               amax_zeroed=True)

    def plain():
        y = F.linear(x, w, bias)
        return F.gelu(y) if epi == 'gelu' else y + res if res is not None else y
    r = alternate(fused, plain, repeats, 1e-5)
    flops = 2 * m * k * n
    return {'name': name, 'M': m, 'K': k, 'N': n, 'epilogue': epi, 'workgroups': -(-m // 32) * (n // 64), **r, 'flops': flops,
            'useful_TFLOPs': flops / r['fused_ms']['median'] / 1e9, 'torch_TFLOPs': flops / r['torch_ms']['median'] / 1e9}


def attention_case(b, heads, n, d, repeats):
    g = torch.Generator(device='cuda').manual_seed(0)
    qkv = torch.randn(b, n, 3, heads, d, device='cuda', generator=g)
    top = torch.zeros(1, device='cuda')

    def plain():
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(b, n, heads * d)
    r = alternate(lambda: ops.attention(qkv, amax_out=top, amax_zeroed=True), plain, repeats, 1e-5)
    return {'B': b, 'heads': heads, 'n': n, 'd': d, **r}


def layer_norm_case(m, c, repeats):
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.randn(m, c, device='cuda', generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(c, device='cuda', generator=g), 0.3 * torch.randn(c, device='cuda', generator=g)
    top = torch.zeros(1, device='cuda')
    r = alternate(lambda: ops.layer_norm(x, gamma, beta, 1e-3, amax_out=top, amax_zeroed=True), lambda: F.layer_norm(x, (c,), gamma, beta, 1e-3), repeats, 1e-5)
    return {'M': m, 'C': c, **r}


def switch_case(module, run, repeats, flag, holder=None):
    """`run(module)` with fused_vit = flag against fused_vit = False on the same module."""
    holder = module if holder is None else holder

    def go(value):
        holder.fused_vit = value
        return run(module)
    return alternate(lambda: go(flag), lambda: go(False), repeats, 1e-4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'vit_bench.json'))
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--views', type=int, default=3)
    ap.add_argument('--skip-producer', action='store_true')
    ap.add_argument('--passes-only', action='store_true', help='the single passes, no modules')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vit_bench: no GPU - nothing is measured without one')
    n, size = args.views, (480, 640)
    m = n * TOKENS
    fmt = lambda s: f"{s['median']:.4f} ({s['min']:.4f}-{s['max']:.4f})"
    line = lambda what, r: print(f"{what}: HIP {fmt(r['fused_ms'])} ms  torch {fmt(r['torch_ms'])} ms  x{r['speedup_median']:.2f}"
                                 f"{'  (spreads overlap)' if r['spreads_overlap'] else ''}", flush=True)
    result = {'device': torch.cuda.get_device_name(0), 'views': n, 'auto_torch_passes': sorted(E.VIT_AUTO_TORCH_PASSES), 'dense': []}
    for name, k, cout, epi in DENSE_SHAPES:
        r = dense_case(name, m, k, cout, epi, args.repeats)
        result['dense'].append(r)
        line(f"dense {name:15s} {m}x{k}->{cout} ({r['workgroups']} workgroups)", r)
    result['attention'] = attention_case(n, HEADS, TOKENS, EMBED // HEADS, args.repeats)
    line(f'attention ({n},{HEADS},{TOKENS},{EMBED // HEADS})', result['attention'])
    result['layer_norm'] = layer_norm_case(m, EMBED, args.repeats)
    line(f'layer_norm {m}x{EMBED}', result['layer_norm'])
    if args.passes_only:
        print(json.dumps(result))
        return
    torch.manual_seed(0)
    tokens_in = torch.randn(n, TOKENS, EMBED, device='cuda')
    block = E.TransformerBlock(HEADS, EMBED).cuda().requires_grad_(False).eval()
    result['block'] = switch_case(block, lambda b: b(tokens_in), args.repeats, True)
    line('one TransformerBlock', result['block'])
    vit = E.VisionTransformer().cuda().requires_grad_(False).eval()
    small = torch.rand(n, 3, 224, 224, device='cuda')
    result['vit'] = switch_case(vit, lambda v: v(small)[-1], args.repeats, True)
    line('VisionTransformer, 12 blocks', result['vit'])
    del block, vit
    images = torch.rand(n, *size, 3, device='cuda')
    per_view = lambda r: {**r, 'fused_ms_per_view': {k: v / n for k, v in r['fused_ms'].items()},
                          'torch_ms_per_view': {k: v / n for k, v in r['torch_ms'].items()}}
    visual = E.VisualFeatures(256, size).cuda().requires_grad_(False).eval()
    result['visual_features'] = per_view(switch_case(visual, lambda v: v(images), args.repeats, 'auto'))
    line("VisualFeatures per call (fused_vit='auto')", result['visual_features'])
    result['visual_features_true'] = per_view(switch_case(visual, lambda v: v(images), args.repeats, True))
    line('VisualFeatures per call (fused_vit=True)', result['visual_features_true'])
    result['stage_split_ms_per_call'] = {}
    for flag in (False, 'auto', True):
        visual.fused_vit = flag
        result['stage_split_ms_per_call'][str(flag)] = s = stage_split(visual, images)
        print(f'stages (fused_vit={flag}, N={n}, ms per call): ' + ', '.join(f'{k} {v:.3f}' for k, v in s.items()), flush=True)
    del visual
    if not args.skip_producer:
        tokens = torch.from_numpy(E.tokenize(['pick up the red block'])).cuda()
        prod = E.LanguageFeatureProducer(size, fused_tail='auto').cuda()
        result['producer'] = per_view(switch_case(prod, lambda p: p(images, tokens=tokens), args.repeats, 'auto', holder=prod.visual_features))
        result['producer']['note'] = ('CLIP is a stand-in (SyntheticCLIPPyramid / SyntheticCLIPText): the producer time excludes the real RN50 '
                                      'and text transformer')
        line("LanguageFeatureProducer per call (fused_vit='auto')", result['producer'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps({'out': args.out}))


if __name__ == '__main__':
    main()
