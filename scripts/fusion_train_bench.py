"""Training through the language fusion (encoders.Conv3x3ActFunction, ops.act_gate, csrc/act_gate.hip, `fused_backward` on
CombineCLIPVisualV4) against the path it replaces - the same convolutions through torch under gradients - on the GPU (fails
without one):

    python scripts/fusion_train_bench.py [--out profiles/fusion_train_bench.json] [--skip-producer]

N = 3 views of 480 x 640.  The four convolutions a gradient crosses on its way to `visual_features`, at the reference's sizes:
up_2 at 120 x 160 (512 + 512 -> 256, elu; 256 -> 256, elu, mul) and up_3 at 240 x 320 (256 + 256 -> 128, elu; 128 -> 128, elu), the
weights frozen and the CLIP half without a gradient.  Per convolution: the backward alone (act gate + data gradient launch against
torch.autograd.grad through a retained torch graph of cat -> conv -> elu -> mul, the same gradient requested) and the forward under
gradients.  Then FeatureProducerV4 forward + backward of `out.square().mean()` per call of 3 views with the fusion's convolutions
HIP in both directions against the same producer with those convolutions through torch; VisualFeatures and the tail run the same way in
both legs (fused_conv='auto', fused_backward=True).  Both legs run in this process, every case warmed up, alternating windows of at least
0.5 s timed with device events, three repeats (median, min - max)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.conv3x3_bwd_bench import alternate, rel  # noqa: E402
from scripts.feature_tail_bwd_bench import peak_above  # noqa: E402
from thesis_clip_nerf_amd import encoders as E  # noqa: E402

CONVS = (('up_2.conv_1', 120, 160, 512, 512, 256, False), ('up_2.conv_2', 120, 160, 256, 0, 256, True),
         ('up_3.conv_1', 240, 320, 256, 256, 128, False), ('up_3.conv_2', 240, 320, 128, 0, 128, False))


def conv_case(name, n, h, w, ca, cb, cout, with_mul, act, repeats):
    gen = torch.Generator(device='cuda').manual_seed(0)
    torch.manual_seed(0)
    conv = E.SameConv2d(ca + cb, cout, 3, bias=False).cuda().requires_grad_(False)
    a = torch.randn(n, h, w, ca, device='cuda', generator=gen).permute(0, 3, 1, 2).requires_grad_(True)
    b = torch.randn(n, h, w, cb, device='cuda', generator=gen).permute(0, 3, 1, 2) if cb else None
    g = torch.randn(n, h, w, cout, device='cuda', generator=gen).permute(0, 3, 1, 2)
    mul = (torch.randn(n, cout, device='cuda', generator=gen) + 1.0)[:, :, None, None] if with_mul else None
    graph = lambda fused: E.conv3x3_act(conv, a, b, act, 'auto', mul, fused_backward=fused)[0]
    out_hip, out_torch = graph(True), graph(False)
    hip_bwd = lambda: torch.autograd.grad(out_hip, [a], g, retain_graph=True)
    torch_bwd = lambda: torch.autograd.grad(out_torch, [a], g, retain_graph=True)
    res = {'name': name, 'N': n, 'h': h, 'w': w, 'Ca': ca, 'Cb': cb, 'Cout': cout, 'act': act, 'mul': with_mul,
           'forward_rel_l2_hip_vs_torch': rel(out_hip.detach(), out_torch.detach()), 'da_rel_l2_hip_vs_torch': rel(hip_bwd()[0], torch_bwd()[0]),
           'flops': 2 * n * h * w * 9 * ca * cout}
    assert res['forward_rel_l2_hip_vs_torch'] < 1e-5 and res['da_rel_l2_hip_vs_torch'] < 1e-4, res      # faster and different is not faster
    res['backward'] = alternate(hip_bwd, torch_bwd, repeats)
    del out_hip, out_torch
    res['forward_under_gradients'] = alternate(lambda: graph(True), lambda: graph(False), repeats)
    return res


def producer_case(n, size, repeats):
    torch.manual_seed(0)
    prod = E.FeatureProducerV4(size, fused_tail='auto', fused_conv='auto', fused_backward=True, fused_visual='auto').cuda()
    fusion = prod.combine_clip_visual
    images = torch.rand(n, *size, 3, device='cuda')

    def step(hip):
        fusion.fused_conv = 'auto' if hip else False                       # under gradients 'auto' without the backward IS torch
        prod.zero_grad(set_to_none=True)
        prod(images).square().mean().backward()

    step(True)
    hip = {k: p.grad.clone() for k, p in prod.named_parameters() if p.grad is not None}
    step(False)
    top = max(float(p.grad.norm()) for p in prod.parameters() if p.grad is not None)
    worst = max(float((hip[k] - p.grad).norm()) for k, p in prod.named_parameters() if p.grad is not None) / top
    r = alternate(lambda: step(True), lambda: step(False), repeats)
    peaks = {'fused': peak_above(lambda: step(True)), 'torch': peak_above(lambda: step(False))}
    return {'N': n, 'size': list(size), 'forward_backward': r, 'peak_MB_forward_backward': peaks,
            'worst_gradient_difference_over_largest_gradient': worst}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'fusion_train_bench.json'))
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--views', type=int, default=3)
    ap.add_argument('--skip-producer', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('fusion_train_bench: no GPU - nothing is measured without one')
    fmt = lambda s: f"{s['median']:.3f} ({s['min']:.3f}-{s['max']:.3f})"
    result = {'device': torch.cuda.get_device_name(0), 'convolutions': [], 'producer': None}
    for name, h, w, ca, cb, cout, with_mul in CONVS:
        r = conv_case(name, args.views, h, w, ca, cb, cout, with_mul, 'elu', args.repeats)
        result['convolutions'].append(r)
        print(f"{name} {ca}+{cb}->{cout} at {h}x{w}: backward HIP {fmt(r['backward']['fused_ms'])} ms torch {fmt(r['backward']['torch_ms'])} ms "
              f"x{r['backward']['speedup_median']:.2f}; forward under gradients {fmt(r['forward_under_gradients']['fused_ms'])} / "
              f"{fmt(r['forward_under_gradients']['torch_ms'])} ms x{r['forward_under_gradients']['speedup_median']:.2f}", flush=True)
    total = lambda leg: sum(r['backward'][leg]['median'] for r in result['convolutions'])
    result['four_backwards_ms'] = {'fused': total('fused_ms'), 'torch': total('torch_ms')}
    print(f"four backwards: HIP {total('fused_ms'):.3f} ms, torch {total('torch_ms'):.3f} ms", flush=True)
    if not args.skip_producer:
        result['producer'] = p = producer_case(args.views, (480, 640), args.repeats)
        print(f"FeatureProducerV4 forward + backward per call of {args.views} views: fusion HIP {fmt(p['forward_backward']['fused_ms'])} ms, torch "
              f"{fmt(p['forward_backward']['torch_ms'])} ms x{p['forward_backward']['speedup_median']:.2f}; peak "
              f"{p['peak_MB_forward_backward']['fused']:.0f} / {p['peak_MB_forward_backward']['torch']:.0f} MB; worst gradient difference / largest "
              f"gradient {p['worst_gradient_difference_over_largest_gradient']:.2g}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps({'out': args.out}))


if __name__ == '__main__':
    main()
