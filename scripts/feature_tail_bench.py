"""The fused feature tail (ops.fuse_upsample2x, csrc/feature_tail.hip) against the torch tail it replaces, and the whole
LanguageFeatureProducer, on the GPU (fails without one):

    python scripts/feature_tail_bench.py [--out profiles/feature_tail_bench.json]

N = 3 views, 240 x 320 -> 480 x 640, (Ca, Cb, act) = (128, 256, elu) [CombineCLIPVisualV4] and (256, 256, identity) [CombineCLIPVisualV0],
fp32 and bf16 output.  The torch tail is what encoders.conv_fusion_tail + the producer do without the kernel: cat -> act -> 1x1 conv ->
interpolate on channels-last NCHW views, then NHWC-contiguous in the output dtype.  Both run in this process, every shape warmed up,
alternating windows of at least 0.5 s timed with device events, three repeats (min / median / max are reported).
Bytes and FLOPs are what the algorithm needs, from the shapes: inputs and weight read once, the output written once, 2 K 256 per
low-resolution pixel (the blend's 6 operations per output element are not counted).  Bound = max(bytes / HBM peak, FLOPs / fp32 MFMA peak)
with the peaks of the hardware guide (8.0 TB/s spec; 6.29 TB/s is what a copy reaches; 157.3 TFLOP/s)."""
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

HBM_PEAK, HBM_COPY, MFMA_F32_PEAK = 8.0e12, 6.29e12, 157.3e12
ACTS = {None: lambda x: x, 'relu': F.relu, 'elu': F.elu}


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


def tail_case(n, h, w, ca, cb, act, dtype, repeats):
    g = torch.Generator(device='cuda').manual_seed(0)
    a = torch.randn(n, h, w, ca, device='cuda', generator=g)
    b = torch.randn(n, h, w, cb, device='cuda', generator=g)
    conv = E.SameConv2d(ca + cb, 256, 1, bias=False).cuda().requires_grad_(False)
    weight = conv.weight.reshape(256, ca + cb).t().contiguous()
    a_nchw, b_nchw = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)               # channels-last views, as the modules hold them
    out = torch.empty(n, 2 * h, 2 * w, 256, dtype=dtype, device='cuda')

    def fused():
        return ops.fuse_upsample2x(a, b, weight, act, out_dtype=dtype, out=out)

    def torch_tail():
        y = E._up(conv(ACTS[act](torch.cat([a_nchw, b_nchw], 1))), 2).permute(0, 2, 3, 1).to(dtype)
        return y if y.is_contiguous() else y.contiguous()

    with torch.no_grad():
        want = torch_tail().float()
        got = fused().float()
        rel = float((got - want).norm() / want.norm())
        assert rel < (1e-5 if dtype == torch.float32 else 4e-3), rel              # faster and different is not faster
        for _ in range(3):
            fused()
            torch_tail()
        torch.cuda.synchronize()
        t_fused, t_torch = [], []
        for _ in range(repeats):
            t_fused.append(window(fused))
            t_torch.append(window(torch_tail))
    esize = 4 if dtype == torch.float32 else 2
    nbytes = n * h * w * (ca + cb) * 4 + (ca + cb) * 256 * 4 + n * 4 * h * w * 256 * esize
    flops = 2 * n * h * w * (ca + cb) * 256
    t_mem, t_mfma = nbytes / HBM_PEAK, flops / MFMA_F32_PEAK
    bound = max(t_mem, t_mfma)
    ms = statistics.median(t_fused)
    return {'N': n, 'h': h, 'w': w, 'Ca': ca, 'Cb': cb, 'act': act or 'identity', 'out_dtype': str(dtype).replace('torch.', ''),
            'fused_ms': spread(t_fused), 'torch_ms': spread(t_torch), 'speedup_median': statistics.median(t_torch) / ms,
            'fused_faster_in_every_repeat': max(t_fused) < min(t_torch), 'rel_l2_fused_vs_torch': rel,
            'bytes': nbytes, 'flops': flops, 'bound_ms': bound * 1e3, 'binds': 'HBM' if t_mem >= t_mfma else 'fp32 MFMA',
            'bound_hbm_ms': t_mem * 1e3, 'bound_mfma_ms': t_mfma * 1e3, 'share_of_bound': bound * 1e3 / ms,
            'achieved_TBps': nbytes / ms / 1e9, 'achieved_TFLOPs': flops / ms / 1e9,
            'share_of_bound_at_copy_bandwidth': max(nbytes / HBM_COPY, t_mfma) * 1e3 / ms}


def producer_case(n, size, repeats):
    """The whole LanguageFeatureProducer per view at `size`, fused tail against torch tail, and where the time goes inside the fusion."""
    torch.manual_seed(0)
    prod = E.LanguageFeatureProducer(size, out_dtype=torch.float32, fused_tail='auto').cuda()
    images = torch.rand(n, size[0], size[1], 3, device='cuda')
    tokens = torch.from_numpy(E.tokenize(['pick up the red block'])).cuda()
    fusion = prod.combine_clip_visual

    def run(fused_tail):
        fusion.fused_tail = fused_tail
        return prod(images, tokens=tokens)

    convs = [m for m in fusion.modules() if isinstance(m, E.SameConv2d) and m.kernel_size == (3, 3)]
    events = []
    hooks = []
    for m in convs:
        def pre(mod, args):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append([e, None])

        def post(mod, args, output):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events[-1][1] = e
        hooks += [m.register_forward_pre_hook(pre), m.register_forward_hook(post)]
    for _ in range(2):
        run('auto')
        run(False)
    torch.cuda.synchronize()
    events.clear()
    run('auto')
    torch.cuda.synchronize()
    conv3_ms = sum(s.elapsed_time(e) for s, e in events)                         # (SameConv2d.forward: the padding copy and the convolution)
    for hk in hooks:
        hk.remove()
    with torch.no_grad():
        visual = prod.visual_features(images)
        pyramid = prod.clip_pyramid(images.permute(0, 3, 1, 2))
        text = prod.clip_text(tokens).expand(n, -1)
    fusion.fused_tail = 'auto'
    with torch.no_grad():
        fusion(pyramid, visual, text)
        torch.cuda.synchronize()
        t_fusion = [window(lambda: fusion(pyramid, visual, text)) for _ in range(repeats)]
    t_auto, t_torch = [], []
    for _ in range(repeats):
        t_auto.append(window(lambda: run('auto')))
        t_torch.append(window(lambda: run(False)))
    per_view = lambda xs: {k: v / n for k, v in spread(xs).items()}
    whole = statistics.median(t_auto)
    return {'N': n, 'H': size[0], 'W': size[1], 'parameters': E.count_parameters(prod),
            'producer_ms_per_view_fused_tail': per_view(t_auto), 'producer_ms_per_view_torch_tail': per_view(t_torch),
            'fusion_ms_per_view_fused_tail': per_view(t_fusion),
            'conv3x3_of_fusion_ms_per_view': conv3_ms / n, 'conv3x3_share_of_producer': conv3_ms / whole,
            'note': 'CLIP is a stand-in (SyntheticCLIPPyramid / SyntheticCLIPText): the producer time excludes the real RN50 and text transformer'}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'feature_tail_bench.json'))
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--views', type=int, default=3)
    ap.add_argument('--size', type=int, nargs=2, default=(480, 640))
    ap.add_argument('--skip-producer', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('feature_tail_bench: no GPU - nothing is measured without one')
    h, w = args.size[0] // 2, args.size[1] // 2
    result = {'device': torch.cuda.get_device_name(0), 'peaks': {'hbm_Bps': HBM_PEAK, 'hbm_copy_Bps': HBM_COPY, 'mfma_f32_flops': MFMA_F32_PEAK},
              'tail': [], 'producer': None}
    for ca, cb, act in ((128, 256, 'elu'), (256, 256, None)):
        for dtype in (torch.float32, torch.bfloat16):
            r = tail_case(args.views, h, w, ca, cb, act, dtype, args.repeats)
            result['tail'].append(r)
            print(f"{ca}+{cb} {r['act']:8s} {r['out_dtype']:8s}: fused {r['fused_ms']['median']:.3f} ms [{r['fused_ms']['min']:.3f}, {r['fused_ms']['max']:.3f}]  "
                  f"torch {r['torch_ms']['median']:.3f} ms [{r['torch_ms']['min']:.3f}, {r['torch_ms']['max']:.3f}]  x{r['speedup_median']:.2f}  "
                  f"bound {r['bound_ms']:.3f} ms ({r['binds']}), share {r['share_of_bound']:.2f}", flush=True)
    result['fused_faster_at_every_shape'] = all(r['fused_faster_in_every_repeat'] for r in result['tail'])
    if not args.skip_producer:
        result['producer'] = p = producer_case(args.views, tuple(args.size), args.repeats)
        print(f"producer per view: {p['producer_ms_per_view_fused_tail']['median']:.2f} ms fused tail, "
              f"{p['producer_ms_per_view_torch_tail']['median']:.2f} ms torch tail; fusion {p['fusion_ms_per_view_fused_tail']['median']:.2f} ms, "
              f"3x3 convolutions {p['conv3x3_of_fusion_ms_per_view']:.2f} ms ({100 * p['conv3x3_share_of_producer']:.0f} % of the producer)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps({'fused_faster_at_every_shape': result['fused_faster_at_every_shape'], 'out': args.out}))


if __name__ == '__main__':
    main()
