"""The backward of the 3x3 convolutions of VisualFeatures as HIP passes (csrc/conv3x3_bwd.hip, encoders.Conv3x3BiasFunction,
`fused_backward`) against the torch path, on the GPU (fails without one):

    python scripts/conv3x3_bwd_bench.py [--out profiles/conv3x3_bwd_bench.json] [--skip-producer]

At N = 3 views and the eight shapes of scripts/visual_features_bench.py: the weight (+ bias) gradient (ops.conv3x3_wgrad, its amax
words given) against aten.convolution_backward with the output mask (False, True, bias), the data gradient (ops.conv3x3 on the
transposed pack; only where the channel counts allow it) against the same call with the mask (True, False, False), and the elementwise
act_in' pass that stays torch.  Then FeatureProducer forward + backward of `out.square().mean()` per call of 3 views at 480 x 640 with
fused_conv='auto' and fused_backward on and off.  Both paths run in this process, every case warmed up, alternating windows of at
least 0.5 s timed with device events, three repeats (median, min - max)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.conv3x3_bench import spread, window  # noqa: E402
from scripts.visual_features_bench import BN_SHAPES, CONV_SHAPES  # noqa: E402
from thesis_clip_nerf_amd import encoders as E  # noqa: E402
from thesis_clip_nerf_amd import ops  # noqa: E402

# name, h, w, Cin, Cout, act_in, bias
SHAPES = [(name, h, w, cin, cout, None, True) for name, h, w, cin, cout, _ in BN_SHAPES] + \
         [(name, h, w, cin, cout, 'relu' if relu_in else None, bias) for name, h, w, cin, cout, relu_in, bias in CONV_SHAPES]


def alternate(fused, torch_path, repeats):
    for _ in range(3):
        fused()
        torch_path()
    torch.cuda.synchronize()
    t_f, t_t = [], []
    for _ in range(repeats):
        t_f.append(window(fused))
        t_t.append(window(torch_path))
    return {'fused_ms': spread(t_f), 'torch_ms': spread(t_t), 'speedup_median': statistics.median(t_t) / statistics.median(t_f),
            'spreads_overlap': not (max(t_f) < min(t_t) or max(t_t) < min(t_f)), 'fused_faster': max(t_f) < min(t_t)}


def rel(a, b):
    return float((a - b).norm() / b.norm())


def conv_case(name, n, h, w, cin, cout, act_in, bias, repeats):
    gen = torch.Generator(device='cuda').manual_seed(0)
    torch.manual_seed(0)
    conv = E.SameConv2d(cin, cout, 3, bias=bias).cuda().requires_grad_(False)
    x = torch.randn(n, h, w, cin, device='cuda', generator=gen)
    g = torch.randn(n, h, w, cout, device='cuda', generator=gen)
    xa = E._ACT_FNS[act_in](x).permute(0, 3, 1, 2)                 # what torch's backward holds: the activated map, channels-last
    g_nchw, x_nchw = g.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2)
    amax_x, amax_g = ops.absmax(x), ops.absmax(g)
    code = E._ACT_CODES[act_in]
    bias_sizes = [cout] if bias else None
    back = lambda mask: torch.ops.aten.convolution_backward(g_nchw, xa, conv.weight, bias_sizes, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, mask)
    nbytes = ops.conv3x3_wgrad_workspace_bytes(n, h, w, cin, cout)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    dw, db = torch.empty(3, 3, cin, cout, device='cuda'), torch.empty(cout, device='cuda')
    out = (dw, db) if bias else dw
    wgrad = lambda: ops.conv3x3_wgrad(x, g, code, amax_x=amax_x, amax_g=amax_g, want_bias=bias, workspace=ws, out=out)
    wgrad()
    want = back([False, True, bias])
    flops = 2 * n * h * w * 9 * cin * cout
    tiles = n * -(-h // 16) * -(-w // 16)
    slabs = -(-tiles // 16)
    res = {'name': name, 'N': n, 'h': h, 'w': w, 'Cin': cin, 'Cout': cout, 'act_in': act_in, 'bias': bias, 'flops': flops, 'slabs': slabs,
           'wgrad_workgroups': slabs * (cin // 32) * (cout // 64), 'workspace_MiB': nbytes / 2 ** 20,
           'wgrad_rel_l2_vs_torch': rel(dw.permute(3, 2, 0, 1), want[1])}
    assert res['wgrad_rel_l2_vs_torch'] < 1e-4, res                       # faster and different is not faster
    res['wgrad'] = r = alternate(wgrad, lambda: back([False, True, bias]), repeats)
    res['wgrad_useful_TFLOPs'], res['wgrad_torch_TFLOPs'] = flops / r['fused_ms']['median'] / 1e9, flops / r['torch_ms']['median'] / 1e9
    if E.conv3x3_dgrad_fusable(conv):
        packed_t = E._packed_conv3x3_t(conv)
        dx = torch.empty(n, h, w, cin, device='cuda')
        dgrad = lambda: ops.conv3x3(g, None, packed_t, cin, 0, amax_a=amax_g, out=dx)
        dgrad()
        res['dgrad_rel_l2_vs_torch'] = rel(dx.permute(0, 3, 1, 2), back([True, False, False])[0])
        assert res['dgrad_rel_l2_vs_torch'] < 1e-4, res
        res['dgrad'] = r = alternate(dgrad, lambda: back([True, False, False]), repeats)
        res['dgrad_workgroups'] = tiles * (cin // 64)
        res['dgrad_useful_TFLOPs'], res['dgrad_torch_TFLOPs'] = flops / r['fused_ms']['median'] / 1e9, flops / r['torch_ms']['median'] / 1e9
        if act_in is not None:
            t = [window(lambda: E.conv3x3_act_grad(dx.permute(0, 3, 1, 2), x_nchw, act_in)) for _ in range(repeats)]
            res['act_grad_ms'] = spread(t)
    else:
        res['dgrad'] = None                                               # torch.nn.grad.conv2d_input in the Function: nothing to compare
    return res


def producer_case(n, size, repeats):
    torch.manual_seed(0)
    prod = E.FeatureProducer(size, fused_conv='auto').cuda()
    images = torch.rand(n, *size, 3, device='cuda')

    def step(flag):
        prod.visual_features.fused_backward = flag
        prod.zero_grad(set_to_none=True)
        prod(images).square().mean().backward()

    def forward_only(flag):
        prod.visual_features.fused_backward = flag
        return prod(images)

    step(True)
    hip = {k: p.grad.clone() for k, p in prod.named_parameters() if p.grad is not None}
    step(False)
    top = max(float(p.grad.norm()) for p in prod.parameters() if p.grad is not None)         # (some true gradients are zero: no ratio per tensor)
    worst = max(float((hip[k] - p.grad).norm()) for k, p in prod.named_parameters() if p.grad is not None) / top
    r = alternate(lambda: step(True), lambda: step(False), repeats)
    f = alternate(lambda: forward_only(True), lambda: forward_only(False), repeats)
    return {'N': n, 'size': list(size), 'forward_backward': r, 'forward_under_gradients': f, 'worst_gradient_difference_over_largest_gradient': worst}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'conv3x3_bwd_bench.json'))
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--views', type=int, default=3)
    ap.add_argument('--skip-producer', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('conv3x3_bwd_bench: no GPU - nothing is measured without one')
    fmt = lambda s: f"{s['median']:.3f} ({s['min']:.3f}-{s['max']:.3f})"
    result = {'device': torch.cuda.get_device_name(0), 'slab_pixels': ops.CONV3X3_WGRAD_SLAB_PIXELS, 'convs': []}
    for shape in SHAPES:
        r = conv_case(shape[0], args.views, *shape[1:], args.repeats)
        result['convs'].append(r)
        line = f"{r['name']:15s} {r['h']}x{r['w']} {r['Cin']}->{r['Cout']}: wgrad HIP {fmt(r['wgrad']['fused_ms'])} ms torch " \
               f"{fmt(r['wgrad']['torch_ms'])} ms x{r['wgrad']['speedup_median']:.2f}"
        if r['dgrad']:
            line += f"; dgrad HIP {fmt(r['dgrad']['fused_ms'])} ms torch {fmt(r['dgrad']['torch_ms'])} ms x{r['dgrad']['speedup_median']:.2f}"
        if 'act_grad_ms' in r:
            line += f"; act' {fmt(r['act_grad_ms'])} ms"
        print(line, flush=True)
    if not args.skip_producer:
        result['producer'] = p = producer_case(args.views, (480, 640), args.repeats)
        print(f"FeatureProducer forward + backward per call of {args.views} views: HIP backward {fmt(p['forward_backward']['fused_ms'])} ms, torch "
              f"{fmt(p['forward_backward']['torch_ms'])} ms; forward under gradients {fmt(p['forward_under_gradients']['fused_ms'])} / "
              f"{fmt(p['forward_under_gradients']['torch_ms'])} ms; worst gradient difference / largest gradient {p['worst_gradient_difference_over_largest_gradient']:.2g}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps({'out': args.out}))


if __name__ == '__main__':
    main()
