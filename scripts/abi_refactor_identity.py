"""Bit identity of two builds of libmvnerf_hip.so on the calls whose host side orchestrates several launches: the training step, the
field backward alone, the query JVP / VJP / fused activations, the grasp-pose optimisation step and the LanguageNeRF training step;
and on the forward field kernels that share the sample front end of mvnerf_field_common.h (forward_legs), with every optional output.
Each library runs in a fresh process (MVNERF_LIB) on the same seeded inputs and prints one SHA-256 per output array; the first library
runs --repeat times, which shows the arrays that are not reproducible from run to run at all (mvnerf_query_vjp sums over the views with
unordered atomics when V > 1, and so does the texel scatter of d_features; with few points a sum has only a few outcomes, hence several
runs).  Those are held, against every run of A, to the bound the existing tests put on that output (bound_for) instead, and are listed.

    python scripts/abi_refactor_identity.py --a variants/lib_parent.so --b thesis_clip_nerf_amd/lib/libmvnerf_hip.so [--out FILE.md]
    python scripts/abi_refactor_identity.py --child OUT.npz [--only steps]       (what the above starts; `steps`: one launch-heavy call each)
"""
import argparse
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda:0'


def child(path, only):
    import torch

    from thesis_clip_nerf_amd import MVVNeRFRenderer, _lib, ops
    from thesis_clip_nerf_amd.synthetic import make_scene
    lib = _lib.lib()
    out = {}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)
    ptr = lambda x: x.data_ptr()

    def ok(rc):
        assert rc == 0, lib.mvnerf_last_error().decode()

    def keep(name, t):
        torch.cuda.synchronize()
        a = t.detach().cpu().numpy().copy()
        if a.nbytes > (8 << 20):                                             # a stash: its digest stands for it
            a = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()
        out[name] = a

    if only != 'steps':
        forward_legs(keep, dev)

    # ---- mvnerf_loss_and_grads / mvnerf_train_step, and mvnerf_field_backward alone on the same scenes ----
    for b, v, full in ((1, 1, False), (2, 2, True)):
        tag = f'B{b}V{v}'
        sc = make_scene(seed=60 + v, batch=b, n_views=v, height=16, width=16, n_rays=32, bias_scale=0.05)
        y = np.random.default_rng(2).random((b, 32, 3)).astype(np.float32)
        ops.texel_table_pays = lambda *a, full=full: full                    # tables (and d_features) on in the second case only
        m = MVVNeRFRenderer(32, 32, n_views=v, batch_size=b, near=sc['near'], far=sc['far'], device=DEV)
        m.set_weights(sc['coarse'], sc['fine'])
        inputs = tuple(sc[k] for k in ['rays_o', 'rays_d', 'images', 'intrinsics', 'extrinsics_inv'])
        u = dict(u_coarse=dev(sc['u_coarse']), u_fine=dev(sc['u_fine']))
        if only == 'steps':
            if full:
                m.compile()
                keep(f'train_step {tag} loss', m.train_step((inputs, y), sc['features'], **u)['loss'])
            continue
        res = m.loss_and_grads(inputs, y, sc['features'], return_d_features=full, **u)
        for name, t in zip(('loss', 'grad', 'rgb', 'depth', 'fine_rgb', 'fine_depth'), (res[0], res[1]) + tuple(res[2])):
            keep(f'loss_and_grads {tag} {name}', t)
        if full:
            keep(f'loss_and_grads {tag} d_features', res[3])
        d = {k: dev(sc[k]) for k in ('rays_o', 'rays_d', 'images', 'features', 'intrinsics', 'extrinsics_inv', 'fine', 'u_coarse')}
        z = ops.stratified_depths(d['u_coarse'], sc['near'], sc['far'])
        geo = (d['rays_o'], d['rays_d'], z, d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'])
        packed, split, streams = ops.pack_net(d['fine']), ops.pack_net_split(d['fine']), ops.pack_bwd_streams(d['fine'])
        table = ops.project_texels(d['features'], packed) if full else None
        rgbs, stash = ops.field_eval_stash(*geo, packed, packed_split=split, texel_table=table)
        d_rgbs = torch.randn(rgbs.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
        grad, d_z, d_feat = f32(ops.NET_PARAMS), f32(b, 32, 64), f32(b, v, 16, 16, 256)
        kw = dict(texel_table=table, texel_grad=f32(b, v, 16, 16, 128)) if full else {}
        ops.field_backward(*geo, d['fine'], streams, stash, rgbs, d_rgbs, grad, d_z=d_z, d_features=d_feat, **kw)
        keep(f'field_backward {tag} stash', stash)
        for name, t in (('grad', grad), ('d_z', d_z), ('d_features', d_feat)):
            keep(f'field_backward {tag} {name}', t)

    # ---- the trunk on query points ----
    for b, v, n in ((1, 1, 40), (2, 3, 64)) if only != 'steps' else ():
        tag = f'B{b}V{v}N{n}'
        sc = make_scene(seed=17 + v, batch=b, n_views=v, height=16, width=20, n_rays=n, bias_scale=0.05)
        rng = np.random.default_rng(117 + v)
        points = (sc['rays_o'] + rng.uniform(sc['near'], sc['far'], (b, n, 1)).astype(np.float32) * sc['rays_d']).astype(np.float32)
        dirs = rng.standard_normal((b, n, 3)).astype(np.float32)
        dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
        tp, td = (dev(rng.standard_normal((b, n, 3)).astype(np.float32) * 1e-2) for _ in range(2))
        g = dev(rng.standard_normal((4, b, n, 128)).astype(np.float32))
        d = {k: dev(sc[k]) for k in ('images', 'features', 'intrinsics', 'extrinsics_inv', 'fine')}
        scene = (d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'])
        packed = ops.pack_net(d['fine'])
        t_acts, acts = ops.query_jvp(dev(points), dev(dirs), tp, td, *scene, packed, return_primal=True)
        stash = ops.query_stash(dev(points), dev(dirs), *scene, packed, packed_split=ops.pack_net_split(d['fine']))
        fused = ops.stash_fused_acts(stash, b, v, n)
        dp, dd = ops.query_vjp(dev(points), dev(dirs), *scene, ops.pack_bwd_streams(d['fine']), stash, g)
        for name, t in (('query_jvp t_acts', t_acts), ('query_jvp acts', acts), ('stash_fused_acts acts', fused), ('query_vjp d_points', dp),
                        ('query_vjp d_dirs', dd)):
            keep(f'{name} {tag}', t)

    # ---- the two pose-driven composite calls, through ctypes: n5 = 7 offsets, P * n5 = 21 rows per scene (32 when padded) ----
    n5, P = 7, 3
    rng = np.random.default_rng(9)
    rnd = lambda *s, scale=0.1: dev((scale * rng.standard_normal(s)).astype(np.float32))
    offsets = np.tile(np.eye(4, dtype=np.float32), (n5, 1, 1))
    offsets[:, :3, 3] = 0.02 * rng.standard_normal((n5, 3))
    offsets = dev(offsets)
    K = 64 * n5
    head = dict(w4=rnd(4, 64, 128), b4=rnd(4, 64), wc=rnd(64, 256), bc=rnd(64))
    tail = [rnd(128, K), rnd(128), rnd(64, 128), rnd(64), rnd(64, K), rnd(64, 64), rnd(64), rnd(64, 64), rnd(64), rnd(1, 64), rnd(1)]

    def poses(n, rd):
        t = (np.array([0.0, 0.0, 0.8]) + 0.1 * rng.standard_normal((n, 3))).astype(np.float32)
        r = rng.standard_normal((n, rd)).astype(np.float32)
        return dev(t), dev(r / np.linalg.norm(r, axis=-1, keepdims=True) if rd == 4 else r)

    def trunk(sc):
        net = dev(sc['fine'])
        return (ops.pack_net(net), ops.pack_net_split(net), ops.pack_bwd_streams(net),
                [dev(sc[k]) for k in ('images', 'features', 'intrinsics', 'extrinsics_inv')])

    for v in (1, 3):                                                            # mvnerf_grasp_opt_step
        sc = make_scene(seed=80 + v, batch=1, n_views=v, height=16, width=20, n_rays=4, bias_scale=0.05)
        packed, split, bwd, scene = trunk(sc)
        head_packed, tail_packed = f32(lib.mvnerf_grasp_head_packed_floats()), f32(lib.mvnerf_grasp_tail_packed_floats(n5))
        ok(lib.mvnerf_grasp_head_pack(ptr(head['w4']), ptr(head['wc']), ptr(head_packed), None))
        ok(lib.mvnerf_grasp_tail_pack(*(ptr(x) for x in tail), n5, ptr(tail_packed), None))
        t, rot = poses(P, 4)
        success, g_t, g_r = f32(1, P), f32(P, 3), f32(P, 4)
        moments = [f32(P, 3), f32(P, 3), f32(P, 4), f32(P, 4)]
        counters, flags = torch.zeros((2, P), dtype=torch.int32, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV)
        ws = torch.zeros(lib.mvnerf_grasp_workspace_bytes(1, v, P, n5), dtype=torch.uint8, device=DEV)
        c = _lib.GraspCall()
        for name, x in (('images', scene[0]), ('features', scene[1]), ('intrinsics', scene[2]), ('extrinsics_inv', scene[3]), ('packed_net', packed),
                        ('split', split), ('bwd_streams', bwd), ('head_packed', head_packed), ('head_b4', head['b4']), ('head_bc', head['bc']),
                        ('tail_packed', tail_packed), ('offsets', offsets), ('t', t), ('rot', rot), ('success', success), ('g_t', g_t),
                        ('g_rot', g_r), ('workspace', ws)):
            setattr(c, name, x.data_ptr())
        c.B, c.V, c.H, c.W, c.rep, c.P, c.n5, c.workspace_bytes = 1, v, 16, 20, 0, P, n5, ws.numel()
        cfg = _lib.PoseAdamConfig()
        cfg.lr0[0], cfg.lr0[1], cfg.decay[0], cfg.decay[1] = 0.05, 0.05, 0.9, 0.09
        cfg.beta1, cfg.beta2, cfg.eps, cfg.clip, cfg.clip_translation = 0.9, 0.999, 1e-7, 1.0, 1
        for i in range(3):
            cfg.lo[i], cfg.hi[i] = -2.0, 2.0
        ok(lib.mvnerf_grasp_opt_step(ctypes.byref(c), ctypes.byref(cfg), ptr(flags), ptr(counters), *(ptr(x) for x in moments), None))
        for name, x in (('success', success), ('g_t', g_t), ('g_rot', g_r), ('t', t), ('rot', rot)):
            keep(f'grasp_opt_step V{v} {name}', x)
        if only == 'steps':
            break

    B = 2
    layout_total = lib.mvnerf_language_grad_floats(n5)
    for v, kind in ((1, 0), (1, 1), (2, 0), (2, 1)) if only != 'steps' else ((2, 0),):      # mvnerf_language_loss_and_grads
        sc = make_scene(seed=50 + v, batch=B, n_views=v, height=16, width=20, n_rays=4, bias_scale=0.05)
        packed, split, bwd, scene = trunk(sc)
        (t1, r1), (t2, r2) = poses(B * P, 6), poses(B * P, 6)
        lab = rng.random((B, P)).astype(np.float32)
        labels = [dev(lab / lab.sum(-1, keepdims=True)), rnd(B, P, 3, scale=1.0), rnd(B, P, 6, scale=1.0)]
        grads, prediction, scalars = f32(layout_total), f32(B, P), f32(4)
        ws = torch.zeros(lib.mvnerf_language_workspace_bytes(B, v, 16, 20, P, n5), dtype=torch.uint8, device=DEV)
        c = _lib.LanguageCall()
        c.images, c.features, c.intrinsics, c.extrinsics_inv = (x.data_ptr() for x in scene)
        c.B, c.V, c.H, c.W = B, v, 16, 20
        c.packed_net, c.split, c.bwd_streams = ptr(packed), ptr(split), ptr(bwd)
        c.head_w4, c.head_b4, c.head_wc, c.head_bc = (ptr(head[k]) for k in ('w4', 'b4', 'wc', 'bc'))
        for i, x in enumerate(tail):
            c.tail_w[i] = ptr(x)
        c.offsets, c.rep, c.np, c.n5 = ptr(offsets), 1, P, n5
        c.t_landscape, c.rot_landscape, c.t_grad, c.rot_grad = ptr(t1), ptr(r1), ptr(t2), ptr(r2)
        c.label_landscape, c.label_grad_t, c.label_grad_r = (ptr(x) for x in labels)
        c.loss_kind, c.w_land, c.w_t, c.w_r = kind, 1.0, 1.0, 1.0
        c.grads, c.prediction, c.scalars = ptr(grads), ptr(prediction), ptr(scalars)
        c.workspace, c.workspace_bytes = ptr(ws), ws.numel()
        ok(lib.mvnerf_language_loss_and_grads(ctypes.byref(c), None))
        for name, x in (('grads', grads), ('prediction', prediction), ('scalars', scalars)):
            keep(f'language_loss_and_grads V{v} {("kl_divergence", "cross_entropy")[kind]} {name}', x)
    assert all(np.isfinite(a.astype(np.float64)).all() for a in out.values()), [k for k, a in out.items() if not np.isfinite(a.astype(np.float64)).all()]
    np.savez(path, **out)
    for k, a in out.items():
        print(f'{hashlib.sha256(a.tobytes()).hexdigest()[:16]}  {k} {a.shape}')


def forward_legs(keep, dev):
    """field_eval, field_eval_split on the 32x32x16 kernel (both direct and through a texel table), field_eval_bf16 (direct) and query_jvp
    on 16x16 maps, B = 2, R = 5, S = 40: 400 samples = 12 whole tiles and one of 16 samples, tiles that straddle rays and the two scenes.
    The stash form with V = 2 needs whole tiles per scene (R * S % 32 == 0): it runs on the first four rays; its stash is zeroed first,
    since a pass leaves the slots nothing reads unwritten."""
    import torch

    from thesis_clip_nerf_amd import ops
    from thesis_clip_nerf_amd.synthetic import make_scene
    k32 = 'split_bf16_32x32x16'
    for v in (1, 2):
        sc = make_scene(seed=70 + v, batch=2, n_views=v, height=16, width=16, n_rays=5, n_samples=40, bias_scale=0.05)
        d = {k: dev(sc[k]) for k in ('rays_o', 'rays_d', 'images', 'features', 'intrinsics', 'extrinsics_inv', 'fine', 'u_coarse')}
        z = ops.stratified_depths(d['u_coarse'], sc['near'], sc['far'])
        scene = (d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'])
        geo = (d['rays_o'], d['rays_d'], z) + scene
        packed, split, packed16 = ops.pack_net(d['fine']), ops.pack_net_split(d['fine']), ops.pack_net_bf16(d['fine'])
        table = ops.project_texels(d['features'], packed)
        wide = dict(return_taps=True, return_pix=True, return_embedding=True, complete_output=True)

        def keep_all(leg, res, names):
            for name, t in zip(names, res):
                for i, x in enumerate(t if isinstance(t, list) else [t]):
                    keep(f'forward V{v} {leg} {name}{i if isinstance(t, list) else ""}', x)

        for form, tab in (('direct', None), ('table', table)):
            keep_all(f'field_eval {form}', ops.field_eval(*geo, packed, texel_table=tab, **wide), ('rgbs', 'tap_idx', 'pix', 'embedding', 'acts'))
            keep_all(f'field_eval_split {form}', ops.field_eval_split(*geo, packed, split, texel_table=tab, kernel=k32, **wide),
                     ('rgbs', 'tap_idx', 'pix', 'embedding', 'acts'))
            r = 5 if v == 1 else 4
            sgeo = (d['rays_o'][:, :r].contiguous(), d['rays_d'][:, :r].contiguous(), z[:, :r].contiguous()) + scene
            zeroed = lambda: torch.zeros(ops.stash_bytes(2, v, r, 40), dtype=torch.uint8, device=DEV)
            keep_all(f'field_eval_stash {form}', ops.field_eval_stash(*sgeo, packed, stash=zeroed(), texel_table=tab), ('rgbs', 'stash'))
            keep_all(f'field_eval_stash split {form}', ops.field_eval_stash(*sgeo, packed, stash=zeroed(), texel_table=tab, packed_split=split,
                                                                            kernel=k32), ('rgbs', 'stash'))
        keep_all('field_eval_bf16 direct', ops.field_eval_bf16(*geo, packed, packed16, return_taps=True, return_embedding=True, return_fused_acts=True),
                 ('rgbs', 'tap_idx', 'embedding', 'fused_acts'))
        rng = np.random.default_rng(31 + v)
        points = ops.points_on_rays(d['rays_o'], d['rays_d'], z).reshape(2, 200, 3).contiguous()
        dirs = d['rays_d'].repeat_interleave(40, dim=1).contiguous()
        tp, td = (dev(rng.standard_normal((2, 200, 3)).astype(np.float32) * 1e-2) for _ in range(2))
        keep_all('query_jvp', ops.query_jvp(points, dirs, tp, td, *scene, packed, return_primal=True), ('t_acts', 'acts'))


def run(lib_path, out_path):
    env = dict(os.environ, MVNERF_LIB=os.path.abspath(lib_path))
    subprocess.run([sys.executable, os.path.abspath(__file__), '--child', out_path], env=env, check=True, stdout=subprocess.DEVNULL)
    with np.load(out_path) as z:
        return {k: z[k] for k in z.files}


def rel_l2(got, ref):
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def query_bars(got, ref):
    """tests/test_gpu_query.py and test_gpu_grasp_optimizer.py, check_close: relative L2 < 3e-2, median relative row error < 3e-3."""
    rows = lambda a: a.reshape(-1, a.shape[-1])
    med = float(np.median(np.linalg.norm(rows(got) - rows(ref), axis=-1) / np.maximum(np.linalg.norm(rows(ref), axis=-1), 1e-30)))
    return rel_l2(got, ref) < 3e-2 and med < 3e-3, f'rel L2 {rel_l2(got, ref):.1e} < 3e-2, median row {med:.1e} < 3e-3'


def net_grad_bars(got, ref):
    """tests/test_gpu_train.py, test_loss_and_grads_match_torch_oracle: per net and section, relative L2 < 6e-3, max |diff| < 3e-2 max |ref|."""
    worst_rel, worst_abs = 0.0, 0.0
    for net in range(got.size // 247300):
        for lo, hi in ((0, 48512), (48512, 48640), (48640, 246784), (246784, 247300)):
            g, r = got[net * 247300 + lo:net * 247300 + hi], ref[net * 247300 + lo:net * 247300 + hi]
            worst_rel = max(worst_rel, rel_l2(g, r))
            worst_abs = max(worst_abs, float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-30)))
    return worst_rel < 6e-3 and worst_abs < 3e-2, f'worst section rel L2 {worst_rel:.1e} < 6e-3, max |diff| / max |ref| {worst_abs:.1e} < 3e-2'


def rel_6e3(got, ref):
    """tests/test_gpu_train.py, test_feature_map_gradient_matches_torch_oracle (the bar without the fine-sample path): relative L2 < 6e-3."""
    return rel_l2(got, ref) < 6e-3, f'rel L2 {rel_l2(got, ref):.1e} < 6e-3'


def abs_bar(bar):
    def check(got, ref):
        err, lim = float(np.abs(got - ref).max()), bar * max(1.0, float(np.abs(ref).max()))
        return err < lim, f'max |diff| {err:.1e} < {lim:.1e}'
    return check


def bound_for(name):
    """The bound the existing tests put on this output (by the last word of its name), for outputs the parent does not reproduce."""
    what = name.split()[-1]
    if what in ('loss', 'rgb', 'depth', 'fine_rgb', 'fine_depth'):
        return abs_bar(1e-5 if what == 'loss' else 1e-4)         # test_gpu_train.py: |loss - ref| < 1e-5, images 1e-4
    if what in ('success', 'prediction', 'scalars'):
        return abs_bar(1e-4)                                     # test_gpu_grasp_step.py / test_gpu_language_step.py: 1e-4 max(1, |ref|)
    if what == 'grad':
        return net_grad_bars
    if what in ('d_features', 'd_z'):
        return rel_6e3
    return query_bars                                            # d_points, d_dirs, g_t, g_rot, t, rot, acts, t_acts, grads (language: 3e-2 |ref|)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--child', default=None)
    ap.add_argument('--only', default=None)
    ap.add_argument('--a', default='variants/lib_parent.so')
    ap.add_argument('--b', default='thesis_clip_nerf_amd/lib/libmvnerf_hip.so')
    ap.add_argument('--repeat', type=int, default=4, help='runs of library A')
    ap.add_argument('--tmp', default='/tmp')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.only)
    *runs_a, b = (run(lib, os.path.join(args.tmp, f'abi_identity_{i}.npz')) for i, lib in enumerate([args.a] * args.repeat + [args.b]))
    a1 = runs_a[0]
    sha = lambda x: hashlib.sha256(x.tobytes()).hexdigest()[:16]
    lines = ['| output | shape | A | B | result |', '|---|---|---|---|---|']
    bad, excepted = [], []
    for k in a1:
        digests = sorted({sha(r[k]) for r in runs_a})
        if len(digests) == 1:
            same = sha(a1[k]) == sha(b[k])
            result = 'identical' if same else 'DIFFERENT'
        else:                                                                # A is not reproducible against itself: the tests' bound,
            check = bound_for(k)                                             # for B against every run of A
            others = [r[k].astype(np.float64) for r in runs_a]
            results = [check(b[k].astype(np.float64), r) for r in others]
            same = all(ok for ok, _ in results)
            shown = ([t for ok, t in results if not ok] or [t for (ok, t), r in zip(results, runs_a) if sha(r[k]) != sha(b[k])] or [results[0][1]])[0]
            a2 = next(r[k].astype(np.float64) for r in runs_a if sha(r[k]) != sha(a1[k]))
            result = (f'A gives {len(digests)} different results in {len(runs_a)} runs ({check(a2, others[0])[1].split(",")[0]} apart); B against '
                      f'every run of A {"inside" if same else "OUTSIDE"} the bound ({shown})' + ('; B equals one of A\'s' if sha(b[k]) in digests else ''))
            excepted.append(k)
        if not same:
            bad.append(k)
        lines.append(f'| {k} | {"x".join(map(str, a1[k].shape)) or "scalar"} | {sha(a1[k])} | {sha(b[k])} | {result} |')
    text = '\n'.join([f'A = `{args.a}` ({args.repeat} runs, the first one shown), B = `{args.b}`; SHA-256 (first 16 hex digits) of every output array.', ''] + lines
                     + ['', f'{len(a1) - len(bad)} of {len(a1)} outputs pass' + (f'; failing: {bad}' if bad else '') + f'; {len(a1) - len(excepted)} bit-identical, '
                        f'{len(excepted)} not reproducible by A itself and held to their tests\' bounds: ' + ', '.join(f'`{k}`' for k in excepted)]) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
