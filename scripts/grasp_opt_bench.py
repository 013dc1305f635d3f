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
--trace N: only N eager steps of the first --step leg after two warm-up steps (for rocprofv3 --kernel-trace: calls / N = launches per step).
--compute-dtype bf16: the A/B of DESIGN.md 12.2 instead of the report above - the fused fp32 step and the fused bf16 step (trunk forward
with relu bits + trunk VJP on the bf16 MFMA) in this one process, both warmed up, in alternating rounds; the trunk stages alone for both;
rel-L2 of success, g_t, g_rot between the two on the same poses.  Writes profiles/grasp_bf16_bench.json (--out) and exits with status 1
unless the bf16 step is faster by more than the spread of the rounds.  With --trace the traced leg uses that compute dtype.
--merge-traces F32_DIR BF16_DIR: no GPU work - reads the *_kernel_trace.csv that two runs of their own
(rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/grasp_opt_bench.py --step fused --compute-dtype DT --trace N)
left in the two directories and adds the per-kernel split, microseconds per step, to the JSON of --out."""
import csv
import glob
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
ap.add_argument('--compute-dtype', choices=['f32', 'bf16'], default='f32')
ap.add_argument('--rounds', type=int, default=7, help='alternating rounds of the --compute-dtype bf16 A/B')
ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'grasp_bf16_bench.json'))
ap.add_argument('--merge-traces', nargs=2, metavar=('F32_DIR', 'BF16_DIR'))
args = ap.parse_args()


def kernel_split(trace_dir):
    """{kernel: [launches per step, us per step]} over the steps of a --trace run (its two warm-up steps included)."""
    acc, steps = {}, 0
    for path in glob.glob(os.path.join(trace_dir, '**', '*_kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r['Kernel_Name'].replace('(anonymous namespace)::', '').split('(')[0].replace('void ', '')
            calls, ns = acc.get(name, (0, 0))
            acc[name] = (calls + 1, ns + int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    steps = acc.get('mvnerf::pose_adam_step_kernel', (0, 0))[0]          # one launch per step
    if not steps:
        raise SystemExit(f'{trace_dir}: no kernel trace of a grasp step')
    return steps, {k: [round(c / steps, 2), round(ns / steps / 1e3, 2)] for k, (c, ns) in sorted(acc.items(), key=lambda kv: -kv[1][1])
                   if k.startswith('mvnerf::')}


if args.merge_traces:
    with open(args.out) as f:
        res = json.load(f)
    for dt, d in zip(('f32', 'bf16'), args.merge_traces):
        steps, split = kernel_split(d)
        res[f'kernels_{dt}'] = {'traced_steps': steps, 'launches_and_us_per_step': split,
                                'sum_us_per_step': round(sum(v[1] for v in split.values()), 1)}
    res['kernels_note'] = ('per kernel of libmvnerf_hip.so: [launches per step, microseconds per step] from rocprofv3 --kernel-trace runs of '
                           'their own (eager fused steps, two of them warm-up); the step times above come from the run without a profiler')
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps({k: res[k] for k in ('kernels_f32', 'kernels_bf16')}))
    sys.exit(0)
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


def optimiser(graph, fused=False, compute_dtype='f32'):
    opt = DNGFOptimizer(model, BOUNDS, n_initial_guesses=P, n_images=NI, clip_translation=True, rotation_representation='6d',
                        compute_dtype=compute_dtype)
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
    opt = optimiser(False, args.step[0] == 'fused', args.compute_dtype)
    for _ in range(2):
        opt.optimize_pose(inputs, feats, [True, False])
    torch.cuda.synchronize()
    for i in range(args.trace):
        opt.optimize_pose(inputs, feats, [i % 2 == 0, i % 2 == 1])
    torch.cuda.synchronize()
    print(json.dumps({'trace_steps': args.trace, 'step': args.step[0], 'compute_dtype': args.compute_dtype, 'poses': P, 'images': NI}))
    sys.exit(0)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def bf16_ab():
    """Fused fp32 step against fused bf16 step, one process, alternating rounds."""
    n5 = model.n_transforms_to_check
    res = {'poses': P, 'images': NI, 'views': 1, 'size': [h, w], 'rotation': '6d', 'query_points_per_step': NI * P * n5, 'reps': args.reps,
           'rounds': args.rounds}
    opts = {dt: optimiser(False, True, dt) for dt in ('f32', 'bf16')}
    # the same poses through both: what the bf16 trunk changes in one step's outputs
    out = {}
    for dt, opt in opts.items():
        s, g_t, g_r = opt.success_and_gradients()
        out[dt] = (s.clone(), g_t.clone(), g_r.clone())
    for i, name in enumerate(('success', 'g_t', 'g_rot')):
        res[f'rel_l2_{name}_bf16_vs_f32'] = rel_l2(out['bf16'][i], out['f32'][i])
    for opt in opts.values():                                # warm-up: every kernel loaded, every buffer sized
        for _ in range(3):
            opt.optimize_pose(inputs, feats, [True, False])
    rounds = {dt: [] for dt in opts}
    for _ in range(args.rounds):
        for dt, opt in opts.items():
            rounds[dt].append(timed(lambda: opt.optimize_pose(inputs, feats, [True, False]), args.reps))
    for dt, v in rounds.items():
        res[f'step_fused_{dt}_ms'] = float(np.median(v))
        res[f'step_fused_{dt}_ms_rounds'] = [round(x, 4) for x in v]
        res[f'step_fused_{dt}_ms_spread'] = float(max(v) - min(v))
    # the two trunk stages alone, on the bound query points of each optimiser
    for dt, opt in opts.items():
        bd, st = opt._bound, opt._bound['state']
        g_acts = torch.randn((4, NI, bd['ld'], 128), generator=gen, device=dev).mul_(1e-3)
        if dt == 'bf16':
            fwd = lambda: ops.query_stash_bf16(bd['points'], bd['dirs'], *st.geo, st.packed, st.packed16, relu_bits=bd['stash'])
            vjp = lambda: ops.query_vjp_bf16(bd['points'], bd['dirs'], *st.geo, st.bwd_streams, st.bwd16, bd['stash'], g_acts)
            g0 = lambda: ops.trunk_vjp_bf16(st.bwd16, bd['stash'], g_acts, 1)
        else:
            def fwd():
                ops.query_stash(bd['points'], bd['dirs'], *st.geo, st.packed, stash=bd['stash'], packed_split=st.packed_split)
                ops.stash_fused_acts(bd['stash'], NI, 1, bd['ld'])
            vjp = lambda: ops.query_vjp(bd['points'], bd['dirs'], *st.geo, st.bwd_streams, bd['stash'], g_acts)
            g0 = None
        for name, fn in (('trunk_fwd', fwd), ('trunk_vjp', vjp), ('trunk_vjp_hidden_layers', g0)):
            if fn is not None:
                fn()
                res[f'{name}_{dt}_ms'] = timed(fn, args.reps)
        res[f'stash_bytes_{dt}'] = int(bd['stash'].numel())
        res[f'grasp_workspace_bytes_{dt}'] = ops.grasp_workspace_bytes(NI, 1, P, n5, bf16=dt == 'bf16')
    gap = res['step_fused_f32_ms'] - res['step_fused_bf16_ms']
    spread = max(res['step_fused_f32_ms_spread'], res['step_fused_bf16_ms_spread'])
    res['step_f32_over_bf16'] = res['step_fused_f32_ms'] / res['step_fused_bf16_ms']
    res['gap_ms'], res['spread_ms'] = gap, spread
    res['bf16_faster_beyond_spread'] = bool(gap > spread)
    res['stages_note'] = ('trunk_fwd_f32 = query_stash + stash_fused_acts (the stash and the re-layout that hands the activations on as rows); '
                          'trunk_fwd_bf16 = query_stash_bf16 alone (it writes rows and relu bits); trunk_vjp_* = the whole input gradient '
                          'incl. the fp32 layer-0 pass; trunk_vjp_hidden_layers_bf16 = trunk_vjp_bf16_kernel alone.  The stages the two steps '
                          'share (pose kernels, head, tail, Adam) are in the per-kernel split (kernels_*), merged from trace runs.')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    return 0 if res['bf16_faster_beyond_spread'] else 1


if args.compute_dtype == 'bf16':
    sys.exit(bf16_ab())

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
