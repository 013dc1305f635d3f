"""bench.py's plain run: only the timed headline (no training legs, no CPU baseline), and `--dump-outputs` writes what the
timed steps computed, which matches the NumPy oracle on every ray."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    from oracle import mvnerf_oracle as O
    from thesis_clip_nerf_amd.synthetic import make_scene

    out = tmp_path / 'outputs'
    proc = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--size', '32',
                           '--dump-outputs', str(out)], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['steps'] == 3 and d['warmup'] == 1 and d['full'] is False and d['unit'] == 'rays/s' and d['higher_is_better'] is True
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 - 32 * 32) < 1e-3 * 32 * 32      # value = 1024 rays per timed step / step time
    for moved in ('train_step', 'train_cfg4', 'cpu_baseline', 'parity'):
        assert moved not in d, moved

    sc = make_scene(seed=0, batch=1, n_views=1, height=32, width=32)                   # the scene bench.py draws on rank 0
    ref = O.render_call(O.unflatten_net(sc['coarse']), O.unflatten_net(sc['fine']), sc['rays_o'], sc['rays_d'], sc['images'],
                        sc['intrinsics'], sc['extrinsics_inv'], sc['features'], sc['near'], sc['far'], sc['n_samples'],
                        sc['u_coarse'], sc['u_fine'])
    assert sorted(os.listdir(out)) == ['depth.npy', 'fine_depth.npy', 'fine_rgb.npy', 'rgb.npy']
    for name, r in zip(['rgb', 'depth', 'fine_rgb', 'fine_depth'], ref):
        got = np.load(out / f'{name}.npy')
        assert got.dtype == np.float32 and got.shape == r.shape, (name, got.dtype, got.shape)
        assert float(np.abs(got - r).max()) < 1e-4, name
