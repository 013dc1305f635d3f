#!/usr/bin/env python3
"""cfg3-shaped workload: the trunk as a field on grasp-pose query points, as train_language.py uses it.
B scenes x (n_points x 42 offsets) query points, V source views of HxW, fp32.  Reports query points/s for
  forward bf16     mvnerf_field_eval_bf16 with the 4 fused activations written (cfg3's dtype)
  forward          mvnerf_field_eval with complete_output (8 activations written)
  forward+stash    what TrunkField.forward runs
  vjp              mvnerf_query_vjp (12 dX launches + layer-0 input gradient)
  jvp              mvnerf_query_jvp (fused primal + tangent pass)
  train_step       LanguageNeRF.train_step: 2 forwards, VJP, JVP, GraspReadout fwd/bwd/double-bwd (per-point layers fused in HIP; per-pose
                   layers through torch + gemm_ops, or fused in HIP with fused_tail), pose algebra and losses in torch, Adam
  train_step (HIP graph)  the same step after compile(graph=True): one graph replay
--fused-tail times the train step with GraspReadout.fused_tail off (today's path) and on, the legs alternating --repeats times, and prints
the median and the range of each leg.  --fused-step adds the leg with compile(fused_step=True) (the step up to the optimiser as one C call,
csrc/language_api.hip) to that alternation; alone it alternates today's path, fused_tail and fused_step.
Usage: python scripts/language_bench.py [--batch 8] [--points 192] [--size 480 640] [--views 1] [--steps 10] [--fused-tail [both|on|off]]
                                        [--fused-step [with|only]] [--repeats 3]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thesis_clip_nerf_amd import ops  # noqa: E402
from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF  # noqa: E402
from thesis_clip_nerf_amd.synthetic import make_scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--points', type=int, default=192, help='poses per scene (x 42 offsets = query points)')
ap.add_argument('--size', type=int, nargs=2, default=[480, 640])
ap.add_argument('--views', type=int, default=1)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--only-train', action='store_true', help='time the train step only (for kernel traces)')
ap.add_argument('--train-mode', choices=['both', 'eager', 'graph'], default='both', help='which train_step legs to run')
ap.add_argument('--fused-tail', nargs='?', const='both', choices=['both', 'on', 'off'], default=None,
                help='time the train step only, with GraspReadout.fused_tail off and on (alternating), or one of the two (for kernel traces)')
ap.add_argument('--fused-step', nargs='?', const='with', choices=['with', 'only'], default=None,
                help='time the train step only: the fused_step leg next to the --fused-tail legs (default: both of them), or alone (for kernel traces)')
ap.add_argument('--repeats', type=int, default=3, help='with --fused-tail / --fused-step: how often each leg is timed (for the spread)')
args = ap.parse_args()
dev = 'cuda:0'
h, w = args.size
sc = make_scene(seed=0, batch=1, n_views=args.views, height=h, width=w, n_rays=4)
rng = np.random.default_rng(0)
b, npts = args.batch, args.points
rep = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).expand(b, *a.shape[1:]).contiguous()
images, feats, k4, einv = rep(sc['images']), rep(sc['features']), rep(sc['intrinsics']), rep(sc['extrinsics_inv'])
model = LanguageNeRF(sc['fine'], n_points_train=npts, n_views=args.views, batch_size=b, rotation_representation='6d',
                     softmax_before_loss=True, device=dev)
model.compile()


def poses():
    t = (np.array([0.0, 0.0, 0.8]) + 0.1 * rng.standard_normal((b, npts, 3))).astype(np.float32)
    return t, rng.standard_normal((b, npts, 6)).astype(np.float32)


t1, r1 = poses()
t2, r2 = poses()
lab0 = rng.random((b, npts)).astype(np.float32)
lab0 /= lab0.sum(-1, keepdims=True)
labels = (lab0, rng.standard_normal((b, npts, 3)).astype(np.float32), rng.standard_normal((b, npts, 6)).astype(np.float32))
inputs = (t1, r1, t2, r2, images, k4, einv)
model.set_pose(t1, r1)
with torch.no_grad():
    tr = model.compute_matrices()
    ps = tr[:, :, None] @ model.transforms_to_check[None, None]
    points = ps[..., :3, 3].reshape(b, -1, 3).contiguous()
    dirs = ps[..., :3, 2].reshape(b, -1, 3).contiguous()
n_q = points.shape[0] * points.shape[1]
state = model.trunk_state(inputs, feats)
geo = state.geo
g_acts = torch.randn(4, b, points.shape[1], 128, device=dev)
tp, td = torch.randn_like(points), torch.randn_like(dirs)
stash = ops.query_stash(points, dirs, *geo, state.packed)


def timed(fn, steps=args.steps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


z0 = torch.zeros(b, points.shape[1], 1, device=dev)
packed16 = ops.pack_net_bf16(model.trunk_net)
eager_steps, graph_steps = max(2, args.steps // 2), max(4, args.steps)


def graph_model(fused_tail=None, fused_step=None):
    """The same step captured as one HIP graph (compile(graph=True)): device-resident inputs bound as the graph's buffers; the two eager steps
    and the capture itself stay outside the timed region."""
    gm = LanguageNeRF(sc['fine'], n_points_train=npts, n_views=args.views, batch_size=b, rotation_representation='6d',
                      softmax_before_loss=True, device=dev)
    gm.compile(graph=True, fused_tail=fused_tail, fused_step=fused_step)
    dv = lambda a: torch.from_numpy(a).to(dev)
    data = ((dv(t1), dv(r1), dv(t2), dv(r2), images, k4, einv), tuple(dv(l) for l in labels))
    gm.bind_graph_inputs(data, feats)
    for _ in range(3):
        gm.train_step(data, feats)
    return gm, data


if args.fused_tail or args.fused_step:
    legs, graphs = {}, {}
    tails = () if args.fused_step == 'only' else {'both': (False, True), 'on': (True,), 'off': (False,)}[args.fused_tail or 'both']
    flags = [(f'fused_tail={fused}', dict(fused_tail=fused, fused_step=False)) for fused in tails]
    if args.fused_step:
        flags.append(('fused_step=True', dict(fused_tail=False, fused_step=True)))
    for _ in range(args.repeats):
        for name, kw in flags:
            if args.train_mode != 'graph':
                model.compile(**kw)
                legs.setdefault(f'train_step, {name}', []).append(timed(lambda: model.train_step((inputs, labels), feats), eager_steps))
            if args.train_mode != 'eager':
                if name not in graphs:
                    graphs[name] = graph_model(**kw)
                gm, data = graphs[name]
                legs.setdefault(f'train_step (HIP graph), {name}', []).append(timed(lambda: gm.train_step(data, feats), graph_steps))
    print(f'B={b} scenes x {points.shape[1]} query points ({npts} poses x 42 offsets), V={args.views}, {h}x{w}; per leg {args.repeats} timings of '
          f'{eager_steps} (eager) / {graph_steps} (graph) steps, alternating')
    for k, ts in sorted(legs.items()):
        ts = sorted(ts)
        print(f'  {k:44s} median {ts[len(ts) // 2] * 1e3:8.3f} ms   min {ts[0] * 1e3:8.3f}   max {ts[-1] * 1e3:8.3f}')
    sys.exit(0)

res = ({'train_step': timed(lambda: model.train_step((inputs, labels), feats), eager_steps)} if args.train_mode != 'graph' else {}) if args.only_train else {
    'forward bf16': timed(lambda: ops.field_eval_bf16(points, dirs, z0, *geo, state.packed, packed16, return_fused_acts=True)),
    'forward': timed(lambda: ops.query_field(points, dirs, *geo, state.packed, complete_output=True)),
    'forward+stash': timed(lambda: ops.query_stash(points, dirs, *geo, state.packed, stash)),
    'vjp': timed(lambda: ops.query_vjp(points, dirs, *geo, state.bwd_streams, stash, g_acts)),
    'jvp': timed(lambda: ops.query_jvp(points, dirs, tp, td, *geo, state.packed)),
    'train_step': timed(lambda: model.train_step((inputs, labels), feats), eager_steps),
}
if args.train_mode != 'eager':
    gmodel, (g_inputs, g_labels) = graph_model()
    res['train_step (HIP graph)'] = timed(lambda: gmodel.train_step((g_inputs, g_labels), feats), graph_steps)
print(f'cfg3 shape: B={b} scenes x {points.shape[1]} query points ({npts} poses x 42 offsets), V={args.views}, {h}x{w}x256 fp32 features '
      f'({feats.numel() * 4 / 1e9:.2f} GB), {n_q} points per pass')
for k, dt in res.items():
    n = 2 * n_q if k.startswith('train_step') else n_q
    print(f'  {k:24s} {dt * 1e3:8.3f} ms   {n / dt / 1e6:8.2f} M query points/s')
