#!/usr/bin/env python3
"""Grasp-pose optimisation at the reference's validation config (configs/validation/grasp_opt_config/3_images.yaml): P = 4096 initial
guesses, n_images = 3 (n_views = 1 -> B = 3 scenes), 480 x 640 source views, 6d rotations (configs/grasp_model/language.yaml),
n_optimization_steps = 16 per phase, init_lr 0.05, decay_t 0.9, decay_r 0.09, clip_translation.  Synthetic scene and weights.
Reports (device events after warm-up):
  step eager       (median of 5 alternating rounds) one DNGFOptimizer.optimize_pose step: pose kernel, trunk forward + stash, fused head, read-out blocks (torch autograd),
                   head VJP, trunk VJP, pose VJP, Adam + post_process
  step graph       the same step as one HIP graph replay (compile(graph=True))
  trunk fwd / vjp  query_stash (+ stash_fused_acts) and query_vjp alone on the same query points (the floor of the step)
  compute_results  wall time of the whole validation call (16 + 16 steps, graph mode), ending in a device synchronise
Usage: python scripts/grasp_opt_bench.py [--poses 4096] [--images 3] [--size 480 640] [--steps 16] [--reps 10] [--step torch fused] [--trace N]
--step: which step runs - torch (stage 4 as torch modules + autograd, the default) and / or fused (compile(fused=True): the whole step
one call of mvnerf_grasp_opt_step).  With both, the four legs (torch / fused x eager / graph) alternate inside every round of one process;
the fused legs report as step_fused_eager_ms / step_fused_graph_ms.
--trace N: only N eager steps of the first --step leg after two warm-up steps (for rocprofv3 --kernel-trace: calls / N = launches per step)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thesis_clip_nerf_amd import ops  # noqa: E402
from thesis_clip_nerf_amd.grasp_optimizer import DNGFOptimizer, compute_results  # noqa: E402
from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF  # noqa: E402
from thesis_clip_nerf_amd.synthetic import make_scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--poses', type=int, default=4096)
ap.add_argument('--images', type=int, default=3)
ap.add_argument('--size', type=int, nargs=2, default=[480, 640])
ap.add_argument('--steps', type=int, default=16, help='n_optimization_steps per phase')
ap.add_argument('--reps', type=int, default=10, help='timed steps per leg')
ap.add_argument('--trace', type=int, default=0)
ap.add_argument('--step', nargs='+', choices=['torch', 'fused'], default=['torch'], help='step legs to time (alternating rounds)')
args = ap.parse_args()
dev = torch.device('cuda:0')
h, w = args.size
P, NI = args.poses, args.images
# the scene's look-at centre is the origin: a workspace around it (the reference's default bounds sit elsewhere in its world frame)
BOUNDS = ((-0.15, 0.15), (-0.15, 0.15), (-0.1, 0.1))
CFG = dict(init_lr_t=0.05, init_lr_r=0.05, decay_t=0.9, decay_r=0.09)

sc = make_scene(seed=0, batch=1, n_views=NI, height=h, width=w, n_rays=4, with_features=False)
gen = torch.Generator(device=dev).manual_seed(0)
feats = torch.randn((1, NI, h, w, 256), generator=gen, device=dev).mul_(0.5)        # N(0, 0.5^2) like make_scene, drawn on the device
inputs = [torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev) for k in ('images', 'intrinsics', 'extrinsics_inv')]
torch.manual_seed(0)
model = LanguageNeRF(sc['fine'], n_views=1, rotation_representation='6d', device=dev)


def optimiser(graph, fused=False):
    opt = DNGFOptimizer(model, BOUNDS, n_initial_guesses=P, n_images=NI, clip_translation=True, rotation_representation='6d')
    opt.compile(graph=graph, fused=fused)
    opt.set_initial_guesses([g[:1] for g in opt.generate_initial_guesses(rng=np.random.default_rng(0))])
    opt.bind(inputs, feats)
    return opt


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


if args.trace:
    opt = optimiser(False, args.step[0] == 'fused')
    for _ in range(2):
        opt.optimize_pose(inputs, feats, [True, False])
    torch.cuda.synchronize()
    for i in range(args.trace):
        opt.optimize_pose(inputs, feats, [i % 2 == 0, i % 2 == 1])
    torch.cuda.synchronize()
    print(json.dumps({'trace_steps': args.trace, 'step': args.step[0], 'poses': P, 'images': NI}))
    sys.exit(0)

n_query = NI * P * model.n_transforms_to_check
res = {'poses': P, 'images': NI, 'views': 1, 'size': [h, w], 'rotation': '6d', 'query_points_per_step': n_query}
steps = list(dict.fromkeys(args.step))
res['step'] = steps
opts = {}
for step in steps:
    prefix = '' if step == 'torch' else 'fused_'
    opts[prefix + 'eager'] = optimiser(False, step == 'fused')
    for _ in range(3):
        opts[prefix + 'eager'].optimize_pose(inputs, feats, [True, False])
    opts[prefix + 'graph'] = optimiser(True, step == 'fused')
    for _ in range(4):
        opts[prefix + 'graph'].optimize_pose(inputs, feats, [True, False])
first = '' if steps[0] == 'torch' else 'fused_'
opt_e, opt_g = opts[first + 'eager'], opts[first + 'graph']
# the legs alternate (5 rounds each): the GPU is shared, so a difference counts only against the spread of its own rounds
legs = {leg: [] for leg in opts}
for _ in range(5):
    for leg, opt in opts.items():
        legs[leg].append(timed(lambda: opt.optimize_pose(inputs, feats, [True, False]), args.reps))
for leg, v in legs.items():
    res[f'step_{leg}_ms'] = float(np.median(v))
    res[f'step_{leg}_ms_rounds'] = [round(x, 4) for x in v]
if 'fused' in steps:
    res['grasp_workspace_bytes'] = ops.grasp_workspace_bytes(NI, 1, P, model.n_transforms_to_check)

# the trunk alone on the bound query points of the eager optimiser
bd, st = opt_e._bound, opt_e._bound['state']
g_acts = torch.randn((4, NI, bd['ld'], 128), generator=gen, device=dev).mul_(1e-3)


def trunk_fwd():
    ops.query_stash(bd['points'], bd['dirs'], *st.geo, st.packed, stash=bd['stash'], packed_split=st.packed_split)
    ops.stash_fused_acts(bd['stash'], NI, 1, bd['ld'])


trunk_fwd()
ops.query_vjp(bd['points'], bd['dirs'], *st.geo, st.bwd_streams, bd['stash'], g_acts)
res['trunk_fwd_stash_ms'] = timed(trunk_fwd, args.reps)
res['trunk_vjp_ms'] = timed(lambda: ops.query_vjp(bd['points'], bd['dirs'], *st.geo, st.bwd_streams, bd['stash'], g_acts), args.reps)

for leg, opt in ((first + 'graph', opt_g), (first + 'eager', opt_e)):
    compute_results(opt, inputs, feats, False, rng=np.random.default_rng(1), n_optimization_steps=2, **CFG)      # warm (same shapes)
    torch.cuda.synchronize()
    t0 = time.time()
    losses_t, losses_r, _, _, duration, _ = compute_results(opt, inputs, feats, False, rng=np.random.default_rng(1),
                                                            n_optimization_steps=args.steps, **CFG)
    torch.cuda.synchronize()
    res[f'compute_results_{leg}_s'] = time.time() - t0
    res[f'compute_results_{leg}_duration_s'] = duration
    res[f'mean_success_after_t_{leg}'] = float(np.mean(losses_t))
    res[f'mean_success_after_r_{leg}'] = float(np.mean(losses_r))
res['pose_steps_per_s'] = P / (res[f'step_{first}graph_ms'] * 1e-3)
res['query_points_per_s'] = n_query / (res[f'step_{first}graph_ms'] * 1e-3)
res['step_over_trunk'] = res[f'step_{first}graph_ms'] / (res['trunk_fwd_stash_ms'] + res['trunk_vjp_ms'])
res['stash_bytes'] = int(bd['stash'].numel())
res['max_memory_allocated_bytes'] = int(torch.cuda.max_memory_allocated(dev))
print(json.dumps(res))
