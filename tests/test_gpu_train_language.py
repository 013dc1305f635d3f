"""The train_language loop on the GPU (thesis_clip_nerf_amd/train_language.py, LanguageNeRF checkpoints in lmvnerf.py): store / load
round trips, a backbone written by MVVNeRFRenderer.store, loading into a captured training graph, device against host batches, and
train_grasp_model end to end (files, resume, best model), at 32 x 32 so that every test takes seconds."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from thesis_clip_nerf_amd import train_language as T
from thesis_clip_nerf_amd.grasp_optimizer import DEFAULT_WORKSPACE_BOUNDS, DNGFOptimizer
from thesis_clip_nerf_amd.lmvnerf import LanguageNeRF, kl_divergence
from thesis_clip_nerf_amd.model import MVVNeRFRenderer
from thesis_clip_nerf_amd.synthetic import glorot_net

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUNDS = DEFAULT_WORKSPACE_BOUNDS
FILES = ('fine_embedding', 'fine_readout', 'grasp_readout')


def make_model(seed, batch=2, paf=2, n_future=6, lr=1e-4, graph=False):
    torch.manual_seed(seed)
    model = LanguageNeRF(glorot_net(np.random.default_rng(seed), bias_scale=0.05), n_points_train=paf * n_future, n_views=1,
                         batch_size=batch, rotation_representation='6d', softmax_before_loss=True, device=DEV)
    model.compile(loss=kl_divergence, learning_rate=lr, graph=graph)
    return model


def make_generator(dataset, batch=2, paf=2, device=DEV, shuffle=True):
    return T.LanguageDataGenerator(dataset, BOUNDS, n_views=1, batch_size=batch, shuffle=shuffle, pose_augmentation_factor=paf,
                                   n_future_poses=6, rotation_representation='6d', device=device)


@pytest.fixture(scope='module')
def dataset():
    return T.SyntheticLanguageDataset(n_scenes=4, n_perspectives=5, height=32, width=32, seed=0)


def state(model):
    return [model.trunk_net.clone()] + [p.detach().clone() for p in model.grasp_readout.parameters()]


def test_store_load_round_trip_and_missing_files(tmp_path):
    a, b = make_model(1), make_model(2)
    path = str(tmp_path / 'ckpt')
    a.store(path)
    assert all(os.path.exists(f'{path}_{f}.pt') for f in FILES)
    params_before = list(b.grasp_readout.parameters())
    trunk_before = b.trunk_net
    assert b.load(path)
    assert all(torch.equal(x, y) for x, y in zip(state(a), state(b)))
    assert b.trunk_net is trunk_before and all(p is q for p, q in zip(params_before, b.grasp_readout.parameters()))   # in place
    c = make_model(3)
    before = state(c)
    os.remove(f'{path}_grasp_readout.pt')
    assert not c.load(path)
    assert c.load_backbone(path)                                   # the backbone alone is still there
    assert torch.equal(c.trunk_net, a.trunk_net)
    assert all(torch.equal(x, y) for x, y in zip(before[1:], state(c)[1:]))
    os.remove(f'{path}_fine_readout.pt')
    assert not c.load_backbone(path, verbose=False) and not c.load(path)


def test_load_backbone_reads_renderer_store(tmp_path):
    renderer = MVVNeRFRenderer(64, 64, n_views=1, device=DEV, seed=5)
    path = str(tmp_path / 'model_final')
    renderer.store(path)
    model = make_model(4)
    assert not torch.equal(model.trunk_net, renderer.fine_net)
    assert model.load_backbone(path)
    assert torch.equal(model.trunk_net, renderer.fine_net)


def test_load_after_graph_capture_reaches_the_replay(tmp_path, dataset):
    """After the capture, `load` must change what the NEXT replay computes: its losses (taken before the step's update) are those of the
    loaded weights, i.e. of an eager model that loaded the same checkpoint (bar: the fp32 rounding of graph against eager, 1e-5)."""
    gen = make_generator(dataset, shuffle=False)
    np.random.seed(0)
    (inputs, features), labels = gen[0]
    graphed = make_model(6, graph=True)
    for _ in range(4):                                             # two eager steps, the capture, one replay
        graphed.train_step((inputs, labels), features)
    assert graphed._graph is not None
    path = str(tmp_path / 'other')
    make_model(7).store(path)
    before = graphed.train_step((inputs, labels), features)
    assert graphed.load(path)
    after = graphed.train_step((inputs, labels), features)
    eager = make_model(8)
    assert eager.load(path)
    want, _ = eager.loss_and_grads((inputs, labels), features)
    for k in want:
        assert abs(float(after[k]) - float(want[k])) < 1e-5 * max(1.0, abs(float(want[k]))), (k, float(after[k]), float(want[k]))
    assert max(abs(float(after[k]) - float(before[k])) for k in want) > 1e-3


def test_device_batches_equal_host_batches(dataset):
    host, device = make_generator(dataset, device=None, shuffle=False), make_generator(dataset, shuffle=False)
    for index in range(len(host)):
        np.random.seed(10 + index)
        (hi, hf), hl = host[index]
        np.random.seed(10 + index)
        (di, df), dl = device[index]
        assert di[7] is None and hi[7] is None
        for h, d in zip(list(hi[:7]) + [hf] + list(hl), list(di[:7]) + [df] + list(dl)):
            assert isinstance(d, torch.Tensor) and d.device == torch.device(DEV) and d.dtype == torch.float32
            assert torch.equal(d.cpu(), torch.from_numpy(h))
    assert len(device._resident) > 0


def _valid(dataset_valid, n):
    return [T.get_inputs(dataset_valid, i, 3, device=DEV) for i in range(n)]


def test_train_grasp_model_end_to_end_and_resume(tmp_path, dataset):
    valid = T.SyntheticLanguageDataset(n_scenes=2, n_perspectives=3, height=32, width=32, seed=1)
    model = make_model(9)
    opt = DNGFOptimizer(model, workspace_bounds=BOUNDS, n_initial_guesses=64, n_images=3, clip_translation=True, rotation_representation='6d')
    config = dict(n_optimization_steps=2, init_lr_t=0.05, init_lr_r=0.05, decay_t=0.9, decay_r=0.09)
    log_dir = str(tmp_path / 'run')
    ckpt = f'{log_dir}/model_final'
    logged, lines = [], []
    np.random.seed(0)
    hist = T.train_grasp_model(model, make_generator(dataset), 2, 1, log_dir, ckpt, opt, config, logged.append, _valid(valid, 2),
                               log=lines.append)
    assert len(hist) == 2 and all(np.isfinite(h[k]) for h in hist for k in h)
    for e in (1, 2):
        with open(f'{log_dir}/valid/results-{e}.pkl', 'rb') as f:
            results = pickle.load(f)
        assert len(results) == 2 and len(results[0]['errors_r']) == 5 and len(results[0]['grasp_poses']) == 5
        assert list(results[0]['final_success']) == sorted(results[0]['final_success'])
    assert [d['epoch'] for d in logged] == [1, 2]
    assert all(os.path.exists(f'{ckpt}_{f}.pt') and os.path.exists(f'{log_dir}/best_{f}.pt') for f in FILES)
    with open(f'{log_dir}/training_progress.json') as f:
        progress = json.load(f)
    assert progress['epoch'] == 2 and T.combined_error(progress['best_mean_error']) < 4000
    # resume: a new process' view - fresh model loaded from the checkpoint, more epochs; only the new epoch is fitted
    resumed = make_model(10)
    assert resumed.load(ckpt)
    assert all(torch.equal(x, y) for x, y in zip(state(resumed), state(model)))
    opt2 = DNGFOptimizer(resumed, workspace_bounds=BOUNDS, n_initial_guesses=64, n_images=3, clip_translation=True,
                         rotation_representation='6d')
    best_mtime = os.path.getmtime(f'{log_dir}/best_grasp_readout.pt')
    hist2 = T.train_grasp_model(resumed, make_generator(dataset), 3, 1, log_dir, ckpt, opt2, config, None, _valid(valid, 2), log=lines.append)
    assert len(hist2) == 1 and os.path.exists(f'{log_dir}/valid/results-3.pkl')
    with open(f'{log_dir}/training_progress.json') as f:
        progress2 = json.load(f)
    assert progress2['epoch'] == 3
    new = np.mean([r['errors_r'][-1] for r in pickle.load(open(f'{log_dir}/valid/results-3.pkl', 'rb'))], axis=0)
    if T.combined_error(new) < T.combined_error(progress['best_mean_error']):
        assert np.allclose(progress2['best_mean_error'], new)
    else:                                                          # the stored best was read back and kept
        assert progress2['best_mean_error'] == progress['best_mean_error']
        assert os.path.getmtime(f'{log_dir}/best_grasp_readout.pt') == best_mtime
    # nothing left to fit: only the opening validation runs
    assert T.train_grasp_model(resumed, make_generator(dataset), 3, 1, log_dir, ckpt, opt2, config, None, _valid(valid, 1), log=lines.append) == []


def test_summed_loss_falls_on_a_fixed_batch(dataset):
    gen = make_generator(dataset, shuffle=False)
    np.random.seed(3)
    (inputs, features), labels = gen[0]
    model = make_model(11, lr=1e-3)
    losses = []
    for _ in range(20):
        out = model.train_step((inputs, labels), features)
        losses.append(float(out['landscape_loss'] + out['grad_loss_t'] + out['grad_loss_r']))
    assert np.isfinite(losses).all()
    assert np.mean(losses[-3:]) < losses[0] - 0.05, losses


def test_graph_fit_history_matches_eager(dataset):
    """fit over the same batches: compile(graph=True) against eager.  Adam turns last-bit differences of small gradient entries into
    lr-sized weight differences (test_gpu_query.py), so the bar on the epoch means is 5e-3 relative, not bit equality."""
    histories = []
    for graph in (False, True):
        model = make_model(12, graph=graph)
        np.random.seed(4)
        histories.append(T.fit(model, make_generator(dataset), 3, log=lambda *_: None))
    for e, g in zip(*histories):
        for k in e:
            assert abs(e[k] - g[k]) < 5e-3 * max(1.0, abs(e[k])), (k, e[k], g[k])
