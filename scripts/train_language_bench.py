"""train_language at the reference shape (batch 8, 32 x 6 = 192 poses per scene, 480 x 640 views, 1 view per scene; validation with
4096 guesses on 3 images, 16 + 16 optimisation steps): ms per training step (eager and one graph replay, batches assembled on the
device beforehand), ms per device batch, seconds per validation sample.  One JSON line.

    python scripts/train_language_bench.py [--size 480x640] [--steps 10] [--fused-tail] [--fused-step] [--rounds 1]

--fused-tail adds the training legs with GraspReadout.fused_tail on (train_step_ms_*_fused_tail, loss_*_fused_tail) after today's legs,
--fused-step those with compile(fused_step=True) (the step up to the optimiser as one C call: train_step_ms_*_fused_step).  With
--rounds N the legs alternate N times in this process and the median is reported (the list of timings as *_all).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thesis_clip_nerf_amd import train_language as T  # noqa: E402
from thesis_clip_nerf_amd.grasp_optimizer import DEFAULT_WORKSPACE_BOUNDS, DNGFOptimizer, compute_results  # noqa: E402
from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF, kl_divergence  # noqa: E402
from thesis_clip_nerf_amd.synthetic import glorot_net  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='480x640')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--guesses', type=int, default=4096)
    ap.add_argument('--fused-tail', action='store_true', help='also time the training step with compile(fused_tail=True)')
    ap.add_argument('--fused-step', action='store_true', help='also time the training step with compile(fused_step=True)')
    ap.add_argument('--rounds', type=int, default=1, help='how often the training legs alternate (the median is reported)')
    args = ap.parse_args()
    h, w = T._size(args.size)
    dev = 'cuda:0'
    t0 = time.time()
    train = T.SyntheticLanguageDataset(args.batch, 3, h, w, seed=0)
    valid = T.SyntheticLanguageDataset(1, 3, h, w, seed=1)
    gen = T.LanguageDataGenerator(train, DEFAULT_WORKSPACE_BOUNDS, n_views=1, batch_size=args.batch, pose_augmentation_factor=32,
                                  n_future_poses=6, rotation_representation='6d', device=dev)
    np.random.seed(0)
    gen.get_data_camera_device(np.arange(args.batch), [np.arange(3)] * args.batch)       # every view resident
    setup_s = time.time() - t0
    torch.cuda.synchronize()
    t0 = time.time()
    batches = [gen[0] for _ in range(args.steps + 3)]
    torch.cuda.synchronize()
    batch_ms = (time.time() - t0) / len(batches) * 1e3
    out = {'size': [h, w], 'batch': args.batch, 'poses_per_scene': 192, 'setup_s': round(setup_s, 1), 'device_batch_ms': round(batch_ms, 2)}
    modes = [('', {})] + ([('_fused_tail', dict(fused_tail=True))] if args.fused_tail else []) + \
        ([('_fused_step', dict(fused_step=True))] if args.fused_step else [])
    timings = {}
    for _ in range(args.rounds):
        for suffix, flags in modes:
            for graph in (False, True):
                torch.manual_seed(0)
                model = LanguageNeRF(glorot_net(np.random.default_rng(0), bias_scale=0.05), n_points_train=192, n_views=1,
                                     batch_size=args.batch, rotation_representation='6d', softmax_before_loss=True, device=dev)
                model.compile(loss=kl_divergence, graph=graph, **flags)
                for (inputs, feats), labels in batches[:3]:
                    model.train_step((inputs, labels), feats)
                torch.cuda.synchronize()
                t0 = time.time()
                for (inputs, feats), labels in batches[3:]:
                    res = model.train_step((inputs, labels), feats)
                torch.cuda.synchronize()
                leg = ('graph' if graph else 'eager') + suffix
                timings.setdefault(leg, []).append((time.time() - t0) / args.steps * 1e3)
                out[f'loss_{leg}'] = float(res['landscape_loss'] + res['grad_loss_t'] + res['grad_loss_r'])
    for leg, ts in timings.items():
        out[f'train_step_ms_{leg}'] = round(sorted(ts)[len(ts) // 2], 2)
        if args.rounds > 1:
            out[f'train_step_ms_{leg}_all'] = [round(t, 2) for t in ts]
    del batches
    model.set_fused_tail(False)                                                               # validation as today
    model.set_fused_step(False)
    data = T.get_inputs(valid, 0, 3, device=dev)
    config = dict(n_optimization_steps=16, init_lr_t=0.05, init_lr_r=0.05, decay_t=0.9, decay_r=0.09)
    for graph in (False, True):
        opt = DNGFOptimizer(model, DEFAULT_WORKSPACE_BOUNDS, n_initial_guesses=args.guesses, n_images=3, clip_translation=True,
                            rotation_representation='6d')
        opt.compile(graph=graph)
        T.validate(opt, config, [data], log=lambda *_: None)                                  # warm-up (and the capture)
        torch.cuda.synchronize()
        t0 = time.time()
        res = T.validate(opt, config, [data, data], log=lambda *_: None)
        out[f'validate_s_per_sample_{"graph" if graph else "eager"}'] = round((time.time() - t0) / 2, 3)
    out['best_error_mm_deg'] = [round(res[-1]['errors_r'][-1][0] * 1000, 1), round(float(np.degrees(res[-1]['errors_r'][-1][1])), 1)]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
