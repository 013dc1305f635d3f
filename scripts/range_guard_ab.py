"""Cost of the range guard on the fine pass of the benchmark's shape (cfg2: one 64x64 source view, 4096 rays x 128 samples, texel-table
form): the guarded fp16 field kernel against the plain one in ONE process, alternating, device events around each leg, and the plain
kernel against itself the same way as the yardstick for the difference.

    python scripts/range_guard_ab.py [--seconds 2.0] [--legs 4] [--out profiles/range_guard_ab.md]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thesis_clip_nerf_amd import ops  # noqa: E402
from thesis_clip_nerf_amd.synthetic import make_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--seconds', type=float, default=2.0, help='at least this much work per variant and leg')
    ap.add_argument('--legs', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('range_guard_ab.py measures on the GPU: none found (not measured)')
    dev = torch.device('cuda:0')
    sc = make_scene(seed=0, batch=1, n_views=1, height=64, width=64)
    d = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev) for k in
         ['rays_o', 'rays_d', 'images', 'features', 'intrinsics', 'extrinsics_inv', 'fine']}
    rng = np.random.default_rng(0)
    z = torch.from_numpy(np.sort(rng.uniform(sc['near'], sc['far'], (1, 4096, 128)).astype(np.float32), -1)).to(dev)
    packed, split = ops.pack_net(d['fine']), ops.pack_net_split(d['fine'])
    table = ops.project_texels(d['features'], packed)
    status = torch.zeros(1, dtype=torch.float32, device=dev)
    call = lambda **kw: ops.field_eval_split(d['rays_o'], d['rays_d'], z, d['images'], d['features'], d['intrinsics'], d['extrinsics_inv'],
                                             packed, split, texel_table=table, **kw)
    variants = {'plain': lambda: call(kernel='split_f16'), 'guarded': lambda: call(kernel='split_f16', range_status=status),
                'plain again': lambda: call(kernel='split_f16')}
    assert torch.equal(variants['plain'](), variants['guarded']())

    def leg(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n                                   # ms per pass

    for fn in variants.values():                                       # warm-up of every variant; sizes the legs
        leg(fn, 20)
    n = max(50, int(args.seconds * 1e3 / leg(variants['plain'], 50)))
    times = {k: [] for k in variants}
    for _ in range(args.legs):
        for k, fn in variants.items():
            times[k].append(leg(fn, n))
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = abs(med['plain again'] / med['plain'] - 1.0)
    lines = ['# Range guard: guarded against plain fp16 field kernel (fine pass of cfg2)', '',
             f'`python scripts/range_guard_ab.py --seconds {args.seconds} --legs {args.legs}` on {torch.cuda.get_device_name(0)}: 4096 rays x 128 samples, one 64x64 source',
             f'view, texel-table form; {n} passes per leg (>= {args.seconds} s), {args.legs} legs per variant, alternating, device events; results bit-identical.', '',
             '| variant | ms per pass (median of legs) | legs |', '|---|---|---|']
    lines += [f'| {k} | {med[k]:.4f} | {", ".join(f"{t:.4f}" for t in times[k])} |' for k in variants]
    lines += ['', f'guarded / plain = {med["guarded"] / med["plain"]:.4f};  plain against itself = {med["plain again"] / med["plain"]:.4f} (spread {100 * spread:.2f} %)',
              f'range status of the pass: {status.item():.6g}']
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
