"""The fused 3x3 convolution (ops.conv3x3, csrc/conv3x3.hip) against the torch path it replaces, on the GPU (fails without one):

    python scripts/conv3x3_bench.py [--out profiles/conv3x3_bench.json] [--skip-producer | --only-producer]

The seven 3x3 convolutions of the reference-sized CombineCLIPVisualV4 at N = 3 views (half size 240 x 320): (h, w, Ca, Cb, Cout, mul).
The torch path is what encoders.py does without the kernel: cat -> F.pad -> conv2d (MIOpen) -> activation -> multiply on channels-last
NCHW views.  Both run in this process, every shape warmed up, alternating windows of at least 0.5 s timed with device events, three
repeats (median, min - max).  The HIP call is given its amax words (in the module they are the previous launch's amax_out) and writes
amax_out.  Executed FLOPs = 3 MFMA products per multiply-add over whole 16 x 16 pixel tiles (the tile-edge excess), as a share of the
2.5 PFLOP/s fp16 peak; bytes = inputs, packed weight stream (6 bytes per weight), mul and output once, against 8.0 TB/s.
Then CombineCLIPVisualV4 on its own and the whole LanguageFeatureProducer per view, with and without fused_conv."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thesis_clip_nerf_amd import encoders as E  # noqa: E402
from thesis_clip_nerf_amd import ops  # noqa: E402

HBM_PEAK, F16_PEAK, TILE = 8.0e12, 2.5e15, 16
# name, h, w, Ca, Cb, Cout, mul
SHAPES = [('conv', 30, 40, 2048, 0, 1024, True), ('up_1.conv_1', 60, 80, 1024, 1024, 512, False), ('up_1.conv_2', 60, 80, 512, 0, 512, True),
          ('up_2.conv_1', 120, 160, 512, 512, 256, False), ('up_2.conv_2', 120, 160, 256, 0, 256, True),
          ('up_3.conv_1', 240, 320, 256, 256, 128, False), ('up_3.conv_2', 240, 320, 128, 0, 128, False)]


def window(fn, min_seconds=0.5):
    """ms per call of fn over a window of at least min_seconds (device events; the count comes from a short calibration)."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(3):
        fn()
    stop.record()
    stop.synchronize()
    n = max(3, int(min_seconds * 1.1 / max(start.elapsed_time(stop) / 3e3, 1e-6)) + 1)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / n


def spread(xs):
    return {'min': min(xs), 'median': statistics.median(xs), 'max': max(xs)}


def conv_case(name, n, h, w, ca, cb, cout, with_mul, repeats):
    g = torch.Generator(device='cuda').manual_seed(0)
    a = torch.randn(n, h, w, ca, device='cuda', generator=g)
    b = torch.randn(n, h, w, cb, device='cuda', generator=g) if cb else None
    mul = torch.randn(n, cout, device='cuda', generator=g) if with_mul else None
    conv = E.SameConv2d(ca + cb, cout, 3, bias=False).cuda().requires_grad_(False)
    packed = ops.conv3x3_pack(conv.weight.permute(2, 3, 1, 0).contiguous())
    amax_a, amax_b = ops.absmax(a), ops.absmax(b) if cb else None
    out, top = torch.empty(n, h, w, cout, device='cuda'), torch.zeros(1, device='cuda')
    a_nchw, b_nchw = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2) if cb else None      # channels-last views, as the modules hold them
    mul4 = mul[:, :, None, None] if with_mul else None

    def fused():
        return ops.conv3x3(a, b, packed, cout, 'elu', mul=mul, amax_a=amax_a, amax_b=amax_b, out=out, amax_out=top)

    def torch_path():
        y = F.elu(conv(torch.cat([a_nchw, b_nchw], 1) if cb else a_nchw))
        return y * mul4 if with_mul else y

    with torch.no_grad():
        want = torch_path().permute(0, 2, 3, 1)
        rel = float((fused() - want).norm() / want.norm())
        assert rel < 1e-5, rel                                                # faster and different is not faster
        for _ in range(3):
            fused()
            torch_path()
        torch.cuda.synchronize()
        t_fused, t_torch = [], []
        for _ in range(repeats):
            t_fused.append(window(fused))
            t_torch.append(window(torch_path))
    k = 9 * (ca + cb)
    flops = 2 * n * h * w * k * cout
    tiles = -(-h // TILE) * -(-w // TILE)
    executed = 3 * 2 * n * tiles * TILE * TILE * k * cout
    nbytes = 4 * n * h * w * (ca + cb + cout) + 6 * k * cout + (4 * n * cout if with_mul else 0)
    ms = statistics.median(t_fused)
    return {'name': name, 'N': n, 'h': h, 'w': w, 'Ca': ca, 'Cb': cb, 'Cout': cout, 'mul': with_mul, 'fused_ms': spread(t_fused),
            'torch_ms': spread(t_torch), 'speedup_median': statistics.median(t_torch) / ms,
            'spreads_overlap': not (max(t_fused) < min(t_torch) or max(t_torch) < min(t_fused)), 'fused_faster': max(t_fused) < min(t_torch),
            'rel_l2_fused_vs_torch': rel, 'flops': flops, 'executed_flops': executed, 'useful_TFLOPs': flops / ms / 1e9,
            'executed_share_of_f16_peak': executed / (ms * 1e-3) / F16_PEAK, 'torch_TFLOPs': flops / statistics.median(t_torch) / 1e9,
            'bytes': nbytes, 'achieved_TBps': nbytes / ms / 1e9, 'hbm_bound_ms': nbytes / HBM_PEAK * 1e3}


def fusion_case(n, repeats):
    """CombineCLIPVisualV4 at the reference's sizes on synthetic inputs, per view, with and without fused_conv."""
    torch.manual_seed(0)
    fusion = E.CombineCLIPVisualV4(use_dense=True, activation='elu', fused_tail='auto').cuda().requires_grad_(False)
    g = torch.Generator(device='cuda').manual_seed(1)
    r = lambda *s: torch.randn(*s, device='cuda', generator=g).contiguous(memory_format=torch.channels_last) if len(s) == 4 else \
        torch.randn(*s, device='cuda', generator=g)
    clip = (r(n, 1024), r(n, 256, 56, 56), r(n, 512, 28, 28), r(n, 1024, 14, 14), r(n, 2048, 7, 7))
    visual, text = r(n, 256, 240, 320), r(n, 1024)

    def run(flag):
        fusion.fused_conv = flag
        return fusion(clip, visual, text)

    with torch.no_grad():
        want, got = run(False), run('auto')
        rel = float((got - want).norm() / want.norm())
        assert rel < 1e-4, rel
        torch.cuda.synchronize()
        t_f, t_t = [], []
        for _ in range(repeats):
            t_f.append(window(lambda: run('auto')))
            t_t.append(window(lambda: run(False)))
    per_view = lambda xs: {k: v / n for k, v in spread(xs).items()}
    return {'N': n, 'fusion_ms_per_view_fused_conv': per_view(t_f), 'fusion_ms_per_view_torch_conv': per_view(t_t),
            'spreads_overlap': not (max(t_f) < min(t_t) or max(t_t) < min(t_f)), 'rel_l2_fused_vs_torch': rel}


def producer_case(n, size, repeats):
    """The whole LanguageFeatureProducer per view at `size`, with and without fused_conv (CLIP is the seeded stand-in)."""
    torch.manual_seed(0)
    prod = E.LanguageFeatureProducer(size, out_dtype=torch.float32, fused_tail='auto').cuda()
    images = torch.rand(n, size[0], size[1], 3, device='cuda')
    tokens = torch.from_numpy(E.tokenize(['pick up the red block'])).cuda()

    def run(flag):
        prod.combine_clip_visual.fused_conv = flag
        return prod(images, tokens=tokens)

    want, got = run(False), run('auto')
    rel = float((got - want).norm() / want.norm())
    assert rel < 1e-4, rel
    torch.cuda.synchronize()
    t_f, t_t = [], []
    for _ in range(repeats):
        t_f.append(window(lambda: run('auto')))
        t_t.append(window(lambda: run(False)))
    per_view = lambda xs: {k: v / n for k, v in spread(xs).items()}
    return {'N': n, 'H': size[0], 'W': size[1], 'producer_ms_per_view_fused_conv': per_view(t_f), 'producer_ms_per_view_torch_conv': per_view(t_t),
            'spreads_overlap': not (max(t_f) < min(t_t) or max(t_t) < min(t_f)), 'rel_l2_fused_vs_torch': rel,
            'note': 'CLIP is a stand-in (SyntheticCLIPPyramid / SyntheticCLIPText): the producer time excludes the real RN50 and text transformer'}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'conv3x3_bench.json'))
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--views', type=int, default=3)
    ap.add_argument('--skip-producer', action='store_true')
    ap.add_argument('--only-producer', action='store_true', help='add the producer to an existing --out file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('conv3x3_bench: no GPU - nothing is measured without one')
    fmt = lambda s: f"{s['median']:.3f} ({s['min']:.3f}-{s['max']:.3f})"
    if args.only_producer:
        with open(args.out) as f:
            result = json.load(f)
    else:
        result = {'device': torch.cuda.get_device_name(0), 'peaks': {'hbm_Bps': HBM_PEAK, 'f16_mfma_flops': F16_PEAK}, 'convs': [],
                  'fusion': None, 'producer': None}
        for name, h, w, ca, cb, cout, with_mul in SHAPES:
            r = conv_case(name, args.views, h, w, ca, cb, cout, with_mul, args.repeats)
            result['convs'].append(r)
            print(f"{name:12s} {h}x{w} {ca}+{cb}->{cout}: HIP {fmt(r['fused_ms'])} ms  torch {fmt(r['torch_ms'])} ms  x{r['speedup_median']:.2f}  "
                  f"useful {r['useful_TFLOPs']:.0f} TF (torch {r['torch_TFLOPs']:.0f}), executed {100 * r['executed_share_of_f16_peak']:.1f} % of f16 peak, "
                  f"{r['achieved_TBps']:.2f} TB/s", flush=True)
        result['convs_total_ms_per_view'] = {k: sum(r[k]['median'] for r in result['convs']) / args.views for k in ('fused_ms', 'torch_ms')}
        print(f"seven convolutions per view: HIP {result['convs_total_ms_per_view']['fused_ms']:.2f} ms, torch {result['convs_total_ms_per_view']['torch_ms']:.2f} ms")
        result['fusion'] = p = fusion_case(args.views, args.repeats)
        print(f"fusion per view: {fmt(p['fusion_ms_per_view_fused_conv'])} ms fused_conv, {fmt(p['fusion_ms_per_view_torch_conv'])} ms torch", flush=True)
    if not args.skip_producer:
        result['producer'] = p = producer_case(args.views, (480, 640), args.repeats)
        print(f"producer per view: {fmt(p['producer_ms_per_view_fused_conv'])} ms fused_conv, {fmt(p['producer_ms_per_view_torch_conv'])} ms torch", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps({'out': args.out}))


if __name__ == '__main__':
    main()
