#!/usr/bin/env python3
"""LanguageNeRF.train_step with its optimiser inside the C call (compile(fused_optimizer=True), csrc/language_opt.hip) against the same
step with torch's Adam (compile(fused_step=True) alone: one clamp per parameter, the foreach Adam, two torch.stack, the trunk packed
every step) - the baseline.  The shape of scripts/language_bench.py: B scenes x (n_points x 42 offsets) query points, V views of HxW, fp32,
6-d rotations, kl_divergence.  The two legs alternate in one process, eager and as a HIP-graph replay, --repeats timings each; the median
and the range of every leg are printed and written to --out as JSON.
--leg torch|fused --train-mode eager|graph runs one leg alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python
scripts/language_opt_bench.py --leg fused --train-mode eager --steps 8 --repeats 1 --out '').
Usage: python scripts/language_opt_bench.py [--batch 8] [--points 192] [--size 480 640] [--views 1] [--steps 200] [--repeats 5]
                                            [--leg both|torch|fused] [--train-mode both|eager|graph] [--out profiles/language_opt_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF  # noqa: E402
from thesis_clip_nerf_amd.synthetic import make_scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--points', type=int, default=192, help='poses per scene (x 42 offsets = query points)')
ap.add_argument('--size', type=int, nargs=2, default=[480, 640])
ap.add_argument('--views', type=int, default=1)
ap.add_argument('--steps', type=int, default=200, help='graph replays per timing (eager: half as many)')
ap.add_argument('--repeats', type=int, default=5, help='timings per leg (for the spread)')
ap.add_argument('--leg', choices=['both', 'torch', 'fused'], default='both')
ap.add_argument('--train-mode', choices=['both', 'eager', 'graph'], default='both')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'language_opt_bench.json'), help="JSON result file ('' for none)")
args = ap.parse_args()
dev = 'cuda:0'
h, w = args.size
b, npts = args.batch, args.points
sc = make_scene(seed=0, batch=1, n_views=args.views, height=h, width=w, n_rays=4)
rng = np.random.default_rng(0)
rep = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).expand(b, *a.shape[1:]).contiguous()
images, feats, k4, einv = rep(sc['images']), rep(sc['features']), rep(sc['intrinsics']), rep(sc['extrinsics_inv'])


def poses():
    t = (np.array([0.0, 0.0, 0.8]) + 0.1 * rng.standard_normal((b, npts, 3))).astype(np.float32)
    return t, rng.standard_normal((b, npts, 6)).astype(np.float32)


t1, r1 = poses()
t2, r2 = poses()
lab0 = rng.random((b, npts)).astype(np.float32)
lab0 /= lab0.sum(-1, keepdims=True)
labels = (lab0, rng.standard_normal((b, npts, 3)).astype(np.float32), rng.standard_normal((b, npts, 6)).astype(np.float32))
dv = lambda a: torch.from_numpy(a).to(dev)
data = ((dv(t1), dv(r1), dv(t2), dv(r2), images, k4, einv), tuple(dv(l) for l in labels))
FLAGS = {'torch': dict(fused_step=True, fused_optimizer=False), 'fused': dict(fused_step=True, fused_optimizer=True)}
NAMES = {'torch': 'fused_step=True, torch Adam (baseline)', 'fused': 'fused_step=True, fused_optimizer=True'}


def make_model(leg, graph):
    model = LanguageNeRF(sc['fine'], n_points_train=npts, n_views=args.views, batch_size=b, rotation_representation='6d',
                         softmax_before_loss=True, device=dev)
    model.compile(graph=graph, **FLAGS[leg])
    if graph:                                   # device-resident inputs bound as the graph's buffers; warm-up and capture stay untimed
        model.bind_graph_inputs(data, feats)
        for _ in range(3):
            model.train_step(data, feats)
    return model


def timed(fn, steps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


eager_steps, graph_steps = max(2, args.steps // 2), max(4, args.steps)
legs = ['torch', 'fused'] if args.leg == 'both' else [args.leg]
modes = ['eager', 'graph'] if args.train_mode == 'both' else [args.train_mode]
models = {(leg, mode): make_model(leg, mode == 'graph') for leg in legs for mode in modes}
timings = {}
for _ in range(args.repeats):
    for leg in legs:                            # the legs alternate
        for mode in modes:
            model = models[leg, mode]
            dt = timed(lambda: model.train_step(data, feats), eager_steps if mode == 'eager' else graph_steps)
            timings.setdefault(f'{mode}: {NAMES[leg]}', []).append(dt * 1e3)
shape = dict(batch=b, poses=npts, offsets=int(models[legs[0], modes[0]].n_transforms_to_check), views=args.views, height=h, width=w,
             eager_steps=eager_steps, graph_steps=graph_steps, repeats=args.repeats)
print(f'B={b} scenes x {npts} poses x {shape["offsets"]} offsets, V={args.views}, {h}x{w}; per leg {args.repeats} timings of {eager_steps} (eager) / '
      f'{graph_steps} (graph) steps, alternating')
result = {'shape': shape, 'device': torch.cuda.get_device_name(0), 'legs': {}}
for k, ts in sorted(timings.items()):
    s = sorted(ts)
    result['legs'][k] = dict(median_ms=round(s[len(s) // 2], 4), min_ms=round(s[0], 4), max_ms=round(s[-1], 4), timings_ms=[round(t, 4) for t in ts])
    print(f'  {k:58s} median {s[len(s) // 2]:8.3f} ms   min {s[0]:8.3f}   max {s[-1]:8.3f}')
if 'fused' in legs:
    print(f'  optimizer steps taken by the fused legs: ' + ', '.join(str(models["fused", m].optimizer_steps()) for m in modes))
if args.out:
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
