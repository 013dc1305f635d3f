"""The backward of the producers' tail as one HIP launch (ops.fuse_upsample2x_bwd, csrc/feature_tail_bwd.hip,
encoders.FuseUpsample2xFunction, `fused_backward` on the combine modules) against torch autograd's backward of the torch
tail, on the GPU (fails without one):

    python scripts/feature_tail_bwd_bench.py [--out profiles/feature_tail_bwd_bench.json] [--skip-producer]

N = 3 views, 240 x 320 -> 480 x 640.  Two cases: (Ca, Cb, act) = (256, 256, identity) with db only and the weight frozen
[CombineCLIPVisualV0 as the reference trains it: the CLIP map has no gradient, the module is in no optimiser] and (128, 256, elu) with
both halves [CombineCLIPVisualV4's tail].  Per case: the backward alone (the fused launch against torch.autograd.grad through a retained
graph of cat -> act -> 1x1 conv -> interpolate on channels-last views, same gradients requested; also torch's time when the weight
gradient is computed too, which is what happens when the module is left unfrozen), the forward under gradients (the Function's forward
against the torch tail's), and torch.cuda.max_memory_allocated above the inputs for forward + backward of each leg.  Then
FeatureProducer forward + backward of `out.square().mean()` per call of 3 views with fused_conv='auto', fused_backward=True, the
combine module frozen, with and without the tail switches.  Both legs run in this process, every case warmed up, alternating windows
of at least 0.5 s timed with device events, three repeats (median, min - max).
Bytes and FLOPs are what the algorithm needs, from the shapes: g read once, X read once where act' needs it, the weight, the requested
gradients written once; 2 x 256 x (requested input channels) per low pixel (the adjoint's 2 x 16 operations per g_low element are listed
apart).  Peaks as in scripts/feature_tail_bench.py."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.conv3x3_bwd_bench import alternate, rel  # noqa: E402
from scripts.feature_tail_bench import HBM_COPY, HBM_PEAK, MFMA_F32_PEAK  # noqa: E402
from thesis_clip_nerf_amd import encoders as E  # noqa: E402
from thesis_clip_nerf_amd import ops  # noqa: E402


def peak_above(fn):
    """max_memory_allocated of fn() above what was allocated before it, in MB."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def tail_case(n, h, w, ca, cb, act, need_a, need_b, repeats):
    gen = torch.Generator(device='cuda').manual_seed(0)
    a = torch.randn(n, h, w, ca, device='cuda', generator=gen)
    b = torch.randn(n, h, w, cb, device='cuda', generator=gen)
    g = torch.randn(n, 2 * h, 2 * w, 256, device='cuda', generator=gen)
    torch.manual_seed(0)
    conv = E.SameConv2d(ca + cb, 256, 1, bias=False).cuda().requires_grad_(False)
    weight = conv.weight.reshape(256, ca + cb).t().contiguous()
    a_nchw, b_nchw = a.permute(0, 3, 1, 2).requires_grad_(need_a), b.permute(0, 3, 1, 2).requires_grad_(need_b)
    g_nchw = g.permute(0, 3, 1, 2)
    wanted = [t for t, need in ((a_nchw, need_a), (b_nchw, need_b)) if need]
    outs = tuple(torch.empty_like(t) if need else None for t, need in ((a, need_a), (b, need_b))) + (None,)

    def graph(fused):
        return E.conv_fusion_tail(a_nchw, b_nchw, conv, act, 'backward' if fused else False)

    out_torch = graph(False)
    fused_bwd = lambda: ops.fuse_upsample2x_bwd(g, a, b, weight, act, need_a, need_b, out=outs)
    torch_bwd = lambda: torch.autograd.grad(out_torch, wanted, g_nchw, retain_graph=True)
    got = [t for t in fused_bwd()[:2] if t is not None]
    want = torch_bwd()
    res = {'N': n, 'h': h, 'w': w, 'Ca': ca, 'Cb': cb, 'act': act or 'identity', 'need_a': need_a, 'need_b': need_b,
           'rel_l2_fused_vs_torch': max(rel(x.permute(0, 3, 1, 2), y) for x, y in zip(got, want))}
    assert res['rel_l2_fused_vs_torch'] < 1e-5, res                       # faster and different is not faster
    res['backward'] = r = alternate(fused_bwd, torch_bwd, repeats)
    conv.requires_grad_(True)                                             # the module left unfrozen: torch also forms the unused weight gradient
    out_w = graph(False)
    with_w = lambda: torch.autograd.grad(out_w, wanted + [conv.weight], g_nchw, retain_graph=True)
    res['backward_torch_with_weight_gradient'] = alternate(fused_bwd, with_w, repeats)['torch_ms']
    conv.requires_grad_(False)
    del out_torch, out_w
    res['forward_under_gradients'] = alternate(lambda: graph(True), lambda: graph(False), repeats)

    def forward_backward(fused):
        a_nchw.grad = b_nchw.grad = None
        graph(fused).backward(g_nchw)

    res['peak_MB_forward_backward'] = {'fused': peak_above(lambda: forward_backward(True)), 'torch': peak_above(lambda: forward_backward(False))}
    a_nchw.grad = b_nchw.grad = None
    k_req = (ca if need_a else 0) + (cb if need_b else 0)
    nbytes = g.numel() * 4 + (n * h * w * k_req * 4 if act else 0) + (ca + cb) * 256 * 4 + n * h * w * k_req * 4
    flops = 2 * n * h * w * 256 * k_req
    ms = r['fused_ms']['median']
    t_mem, t_mfma = nbytes / HBM_PEAK, flops / MFMA_F32_PEAK
    res.update({'bytes': nbytes, 'flops': flops, 'adjoint_flops': 32 * n * h * w * 256, 'bound_hbm_ms': t_mem * 1e3, 'bound_mfma_ms': t_mfma * 1e3,
                'bound_sum_ms': (t_mem + t_mfma) * 1e3, 'share_of_bound_sum': (t_mem + t_mfma) * 1e3 / ms,
                'bound_sum_at_copy_bandwidth_ms': (nbytes / HBM_COPY + t_mfma) * 1e3, 'achieved_TBps': nbytes / ms / 1e9,
                'achieved_TFLOPs': flops / ms / 1e9, 'workgroups': n * -(-h // 8) * -(-w // 16)})
    return res


def producer_case(n, size, repeats):
    torch.manual_seed(0)
    prod = E.FeatureProducer(size, fused_conv='auto', fused_backward=True).cuda()
    tail = prod.combine_clip_visual.requires_grad_(False)                 # in no optimiser (FeatureProducer.trainable_parameters)
    images = torch.rand(n, *size, 3, device='cuda')

    def step(flag):
        tail.fused_tail, tail.fused_backward = ('auto', True) if flag else (False, False)
        prod.zero_grad(set_to_none=True)
        prod(images).square().mean().backward()

    step(True)
    hip = {k: p.grad.clone() for k, p in prod.named_parameters() if p.grad is not None}
    step(False)
    top = max(float(p.grad.norm()) for p in prod.parameters() if p.grad is not None)         # (some true gradients are zero: no ratio per tensor)
    worst = max(float((hip[k] - p.grad).norm()) for k, p in prod.named_parameters() if p.grad is not None) / top
    r = alternate(lambda: step(True), lambda: step(False), repeats)
    peaks = {'fused': peak_above(lambda: step(True)), 'torch': peak_above(lambda: step(False))}
    return {'N': n, 'size': list(size), 'forward_backward': r, 'peak_MB_forward_backward': peaks,
            'worst_gradient_difference_over_largest_gradient': worst}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'feature_tail_bwd_bench.json'))
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--views', type=int, default=3)
    ap.add_argument('--size', type=int, nargs=2, default=(480, 640))
    ap.add_argument('--skip-producer', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('feature_tail_bwd_bench: no GPU - nothing is measured without one')
    fmt = lambda s: f"{s['median']:.3f} ({s['min']:.3f}-{s['max']:.3f})"
    h, w = args.size[0] // 2, args.size[1] // 2
    result = {'device': torch.cuda.get_device_name(0), 'peaks': {'hbm_Bps': HBM_PEAK, 'hbm_copy_Bps': HBM_COPY, 'mfma_f32_flops': MFMA_F32_PEAK},
              'tail': [], 'producer': None}
    for ca, cb, act, need_a, need_b in ((256, 256, None, False, True), (128, 256, 'elu', True, True)):
        r = tail_case(args.views, h, w, ca, cb, act, need_a, need_b, args.repeats)
        result['tail'].append(r)
        print(f"{ca}+{cb} {r['act']:8s} need_a={need_a}: backward HIP {fmt(r['backward']['fused_ms'])} ms torch {fmt(r['backward']['torch_ms'])} ms "
              f"x{r['backward']['speedup_median']:.2f} (torch with the weight gradient {fmt(r['backward_torch_with_weight_gradient'])} ms); forward under "
              f"gradients {fmt(r['forward_under_gradients']['fused_ms'])} / {fmt(r['forward_under_gradients']['torch_ms'])} ms; peak "
              f"{r['peak_MB_forward_backward']['fused']:.0f} / {r['peak_MB_forward_backward']['torch']:.0f} MB; bounds HBM {r['bound_hbm_ms']:.3f} + MFMA "
              f"{r['bound_mfma_ms']:.3f} ms, share {r['share_of_bound_sum']:.2f}", flush=True)
    if not args.skip_producer:
        result['producer'] = p = producer_case(args.views, tuple(args.size), args.repeats)
        print(f"FeatureProducer forward + backward per call of {args.views} views: tail switches on {fmt(p['forward_backward']['fused_ms'])} ms, off "
              f"{fmt(p['forward_backward']['torch_ms'])} ms; peak {p['peak_MB_forward_backward']['fused']:.0f} / {p['peak_MB_forward_backward']['torch']:.0f} MB; "
              f"worst gradient difference / largest gradient {p['worst_gradient_difference_over_largest_gradient']:.2g}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps({'out': args.out}))


if __name__ == '__main__':
    main()
