"""VisualFeatures with its 3x3 convolutions and batch-statistics normalisations as HIP passes (encoders.py `fused_conv`; csrc/conv3x3.hip,
csrc/batchnorm.hip) against the torch path, on the GPU (fails without one):

    python scripts/visual_features_bench.py [--out profiles/visual_features_bench.json] [--skip-producer]

At N = 3 views of 480 x 640, the reference's sizes: the distinct convolution + normalisation shapes of the conv encoder's blocks
(240 x 320: 64 -> 128 and 128 -> 128 with relu, 128 -> 128 with skip and relu), the two `output_conv` convolutions (112 x 112,
relu in front, bias), the `conv_decode` convolutions the kernel takes (28 x 28 ... 7 x 7, to 256 channels), then VisualFeatures alone
and the whole LanguageFeatureProducer per view with and without the switch, and one run under forward hooks for the per-stage split of
VisualFeatures (conv encoder / ViT / decoder).  The torch path is what encoders.py does without the kernels (conv2d through MIOpen on
channels-last views, F.batch_norm with batch statistics, add, relu).  Both paths run in this process, every shape warmed up,
alternating windows of at least 0.5 s timed with device events, three repeats (median, min - max)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.conv3x3_bench import spread, window  # noqa: E402
from thesis_clip_nerf_amd import encoders as E  # noqa: E402

# name, h, w, Cin, Cout, skip: convolution (bias) -> batch-statistics normalisation -> (skip) -> relu
BN_SHAPES = [('block_1.conv_1', 240, 320, 64, 128, False), ('block.conv_1', 240, 320, 128, 128, False), ('block.conv_2', 240, 320, 128, 128, True)]
# name, h, w, Cin, Cout, relu in front, bias
CONV_SHAPES = [('output_conv.1', 112, 112, 1024, 256, True, True), ('output_conv.3', 112, 112, 256, 128, True, True),
               ('conv_decode.1', 28, 28, 96, 256, False, False), ('conv_decode.2', 14, 14, 192, 256, False, False),
               ('conv_decode.3', 7, 7, 384, 256, False, False)]


def alternate(fused, torch_path, repeats, tol):
    """Checks the two paths against each other, warms both up, then alternating windows -> the result fields both kinds of case share."""
    with torch.no_grad():
        want, got = torch_path(), fused()
        rel = float((got - want).norm() / want.norm())
        assert rel < tol, rel                                                 # faster and different is not faster
        for _ in range(3):
            fused()
            torch_path()
        torch.cuda.synchronize()
        t_f, t_t = [], []
        for _ in range(repeats):
            t_f.append(window(fused))
            t_t.append(window(torch_path))
    return {'fused_ms': spread(t_f), 'torch_ms': spread(t_t), 'speedup_median': statistics.median(t_t) / statistics.median(t_f),
            'spreads_overlap': not (max(t_f) < min(t_t) or max(t_t) < min(t_f)), 'fused_faster': max(t_f) < min(t_t),
            'rel_l2_fused_vs_torch': rel}


def bn_case(name, n, h, w, cin, cout, with_skip, repeats):
    torch.manual_seed(0)
    conv = E.SameConv2d(cin, cout, 3).cuda().requires_grad_(False)
    norm = E._keras_bn(cout).cuda().requires_grad_(False)
    g = torch.Generator(device='cuda').manual_seed(0)
    with torch.no_grad():
        conv.bias.copy_(0.2 * torch.randn(cout, device='cuda', generator=g))
        norm.weight.copy_(1 + 0.3 * torch.randn(cout, device='cuda', generator=g))
        norm.bias.copy_(0.3 * torch.randn(cout, device='cuda', generator=g))
    x = torch.randn(n, h, w, cin, device='cuda', generator=g).permute(0, 3, 1, 2)         # channels-last views, as the modules hold them
    skip = torch.randn(n, h, w, cout, device='cuda', generator=g).permute(0, 3, 1, 2) if with_skip else None
    amax = x.abs().max().reshape(1)                                            # in the module it is the previous apply's amax_out
    r = alternate(lambda: E.conv3x3_bn(conv, norm, x, skip, True, amax)[0], lambda: E.conv3x3_bn(conv, norm, x, skip, False)[0], repeats, 1e-5)
    flops = 2 * n * h * w * 9 * cin * cout
    return {'name': name, 'N': n, 'h': h, 'w': w, 'Cin': cin, 'Cout': cout, 'skip': with_skip, **r, 'flops': flops,
            'useful_TFLOPs': flops / r['fused_ms']['median'] / 1e9, 'torch_TFLOPs': flops / r['torch_ms']['median'] / 1e9}


def conv_case(name, n, h, w, cin, cout, relu_in, bias, repeats):
    torch.manual_seed(0)
    conv = E.SameConv2d(cin, cout, 3, bias=bias).cuda().requires_grad_(False)
    g = torch.Generator(device='cuda').manual_seed(0)
    if bias:
        with torch.no_grad():
            conv.bias.copy_(0.2 * torch.randn(cout, device='cuda', generator=g))
    x = torch.randn(n, h, w, cin, device='cuda', generator=g).permute(0, 3, 1, 2)
    amax = x.abs().max().reshape(1)
    act_in = 'relu' if relu_in else None
    if bias:
        fused, plain = (lambda: E.conv3x3_bias(conv, x, act_in, True, amax)[0]), (lambda: E.conv3x3_bias(conv, x, act_in, False)[0])
    else:
        fused, plain = (lambda: E.conv3x3_act(conv, x, None, None, True, amax_a=amax)[0]), (lambda: E.conv3x3_act(conv, x, None, None, False)[0])
    r = alternate(fused, plain, repeats, 1e-5)
    flops = 2 * n * h * w * 9 * cin * cout
    return {'name': name, 'N': n, 'h': h, 'w': w, 'Cin': cin, 'Cout': cout, 'relu_in': relu_in, 'bias': bias, **r, 'flops': flops,
            'useful_TFLOPs': flops / r['fused_ms']['median'] / 1e9, 'torch_TFLOPs': flops / r['torch_ms']['median'] / 1e9}


def stage_split(visual, images, iterations=20):
    """ms per call of the stages of VisualFeatures under forward hooks (device events around conv_features, vision_transformer and its
    vit): decoder = vision_transformer - vit, rest = the two resizes and the concat."""
    stages = {'conv_encoder': visual.conv_features, 'vit_encoder': visual.vision_transformer, 'vit': visual.vision_transformer.vit}
    events, handles = {k: [] for k in stages}, []
    for key, module in stages.items():
        def pre(_m, _a, key=key):
            e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            events[key].append(e)
            e[0].record()
        handles.append(module.register_forward_pre_hook(pre))
        handles.append(module.register_forward_hook(lambda _m, _a, _o, key=key: events[key][-1][1].record()))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        visual(images)
        for v in events.values():
            v.clear()
        start.record()
        for _ in range(iterations):
            visual(images)
        stop.record()
    torch.cuda.synchronize()
    for hnd in handles:
        hnd.remove()
    ms = {k: sum(a.elapsed_time(b) for a, b in v) / iterations for k, v in events.items()}
    total = start.elapsed_time(stop) / iterations
    return {'conv_encoder': ms['conv_encoder'], 'vit': ms['vit'], 'decoder': ms['vit_encoder'] - ms['vit'],
            'rest': total - ms['conv_encoder'] - ms['vit_encoder'], 'total': total}


def module_case(make, run, n, repeats, key):
    module = make()

    def go(flag):
        module.visual_features.fused_conv = flag
        return run(module)

    r = alternate(lambda: go('auto'), lambda: go(False), repeats, 1e-4)
    per_view = lambda s: {k: v / n for k, v in s.items()}
    return module, {'N': n, f'{key}_ms_per_view_fused': per_view(r['fused_ms']), f'{key}_ms_per_view_torch': per_view(r['torch_ms']),
                    'spreads_overlap': r['spreads_overlap'], 'rel_l2_fused_vs_torch': r['rel_l2_fused_vs_torch']}


class _Visual(torch.nn.Module):
    """VisualFeatures under the attribute name the producer uses, so module_case drives both."""

    def __init__(self, size):
        super().__init__()
        self.visual_features = E.VisualFeatures(256, size)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'visual_features_bench.json'))
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--views', type=int, default=3)
    ap.add_argument('--skip-producer', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('visual_features_bench: no GPU - nothing is measured without one')
    n, size = args.views, (480, 640)
    fmt = lambda s: f"{s['median']:.3f} ({s['min']:.3f}-{s['max']:.3f})"
    result = {'device': torch.cuda.get_device_name(0), 'conv_bn': [], 'convs': []}
    for name, h, w, cin, cout, skip in BN_SHAPES:
        r = bn_case(name, n, h, w, cin, cout, skip, args.repeats)
        result['conv_bn'].append(r)
        print(f"{name:15s} {h}x{w} {cin}->{cout} skip={skip}: HIP {fmt(r['fused_ms'])} ms  torch {fmt(r['torch_ms'])} ms  x{r['speedup_median']:.2f}", flush=True)
    for name, h, w, cin, cout, relu_in, bias in CONV_SHAPES:
        r = conv_case(name, n, h, w, cin, cout, relu_in, bias, args.repeats)
        result['convs'].append(r)
        print(f"{name:15s} {h}x{w} {cin}->{cout}: HIP {fmt(r['fused_ms'])} ms  torch {fmt(r['torch_ms'])} ms  x{r['speedup_median']:.2f}", flush=True)
    torch.manual_seed(0)
    images = torch.rand(n, *size, 3, device='cuda')
    holder, result['visual_features'] = module_case(lambda: _Visual(size).cuda().requires_grad_(False).eval(),
                                                    lambda m: m.visual_features(images), n, args.repeats, 'visual')
    p = result['visual_features']
    print(f"VisualFeatures per view: {fmt(p['visual_ms_per_view_fused'])} ms fused, {fmt(p['visual_ms_per_view_torch'])} ms torch", flush=True)
    result['stage_split_ms_per_call'] = {}
    for flag in (False, 'auto'):
        holder.visual_features.fused_conv = flag
        result['stage_split_ms_per_call'][str(flag)] = s = stage_split(holder.visual_features, images)
        print(f'stages (fused_conv={flag}, N={n}, ms per call): ' + ', '.join(f'{k} {v:.3f}' for k, v in s.items()), flush=True)
    del holder
    if not args.skip_producer:
        tokens = torch.from_numpy(E.tokenize(['pick up the red block'])).cuda()
        for fused_conv in (False, 'auto'):
            _, p = module_case(lambda: E.LanguageFeatureProducer(size, fused_tail='auto', fused_conv=fused_conv).cuda(),
                               lambda m: m(images, tokens=tokens), n, args.repeats, 'producer')
            p['note'] = 'CLIP is a stand-in (SyntheticCLIPPyramid / SyntheticCLIPText): the producer time excludes the real RN50 and text transformer'
            result[f'producer_fused_conv_{fused_conv}'] = p
            print(f"producer per view (fusion fused_conv={fused_conv}): {fmt(p['producer_ms_per_view_fused'])} ms fused_visual, "
                  f"{fmt(p['producer_ms_per_view_torch'])} ms torch visual", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps({'out': args.out}))


if __name__ == '__main__':
    main()
