"""The train_language loop's host side (thesis_clip_nerf_amd/train_language.py) without a GPU: the generator against a straight NumPy +
scipy restatement of data_generator/language.py and manipulation_tasks' Affine, the restated scipy rotations, the label layout and the
pose split, grasp_error against closed forms, the validation bookkeeping (get_step_results, log_results, load_training_progress, the
best-model rule), the checkpoint importer and the cross-entropy loss."""
import json
import math

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from thesis_clip_nerf_amd import train_language as T
from thesis_clip_nerf_amd.encoders import load_grasp_readout
from thesis_clip_nerf_amd.grasp_optimizer import DEFAULT_WORKSPACE_BOUNDS
from thesis_clip_nerf_amd.lmvnerf import GraspReadout, categorical_crossentropy_from_logits
from thesis_clip_nerf_amd.model import camera_parameters

BOUNDS = DEFAULT_WORKSPACE_BOUNDS


# ---- the reference, restated with scipy (transform.py:11-55, language.py:36-167) ------------------------------------------------------
class Affine:
    def __init__(self, translation=(0, 0, 0), rotation=(0, 0, 0, 1)):
        self.matrix = np.eye(4)
        self.matrix[:3, 3] = np.array(translation)
        if len(rotation) == 4:
            self.matrix[:3, :3] = Rotation.from_quat(rotation).as_matrix()
        else:
            self.matrix[:3, :3] = Rotation.from_euler('xyz', rotation).as_matrix()

    @classmethod
    def from_matrix(cls, matrix):
        a = cls()
        a.matrix = matrix
        return a

    @classmethod
    def random(cls, t_bounds=((0, 1), (0, 1), (0, 1)), r_bounds=((0, 2 * np.pi), (0, 2 * np.pi), (0, 2 * np.pi)),
               allow_zero_rotation=True):
        t_b = np.array(t_bounds)
        translation = np.random.uniform(t_b[:, 0], t_b[:, 1])
        r_b = np.array(r_bounds)
        rpy = np.array([0.0, 0.0, 0.0])
        if not allow_zero_rotation:
            while (rpy < 0.0001).all():
                rpy = np.random.uniform(r_b[:, 0], r_b[:, 1])
        else:
            rpy = np.random.uniform(r_b[:, 0], r_b[:, 1])
        return cls(translation=translation, rotation=Rotation.from_euler('xyz', rpy).as_quat())

    @property
    def translation(self):
        return self.matrix[:3, 3]

    @property
    def rotation(self):
        return self.matrix[:3, :3]

    @property
    def quat(self):
        return Rotation.from_matrix(self.matrix[:3, :3]).as_quat()


def reference_batch(ds, batch, n_views, paf, n_future, fixed_orientation, representation):
    n_points = n_future * paf
    if fixed_orientation is not None:
        n_negative, n_r_negative = n_points - n_future, 0
    else:
        n_negative = (7 * n_points) // 8 - n_future
        n_r_negative = n_points - n_negative - n_future
    rot = (lambda p: Affine.from_matrix(p).quat) if representation == 'quaternion' else (
        lambda p: np.concatenate([Affine.from_matrix(p).rotation[:, 0], Affine.from_matrix(p).rotation[:, 1]]))
    imgs, ks, es = [], [], []
    for i in batch:                                                               # get_data_camera
        src = np.random.choice(range(ds.n_perspectives), size=n_views, replace=False)
        cams = [camera_parameters(ds.cameras[i][s]) for s in src]
        imgs.append([ds.colors[i][s][..., :3] / 255.0 for s in src])
        es.append([c[0] for c in cams])
        ks.append([c[1] for c in cams])
    lt, lr, labels = [], [], []
    for i in batch:                                                               # get_data_landscape_final
        target_pose = ds.grasp_poses[i]
        negative = [Affine.random(BOUNDS).matrix for _ in range(n_negative + n_future - 1)]
        r_tf = [Affine.random(t_bounds=((-0.01, 0.01),) * 3, allow_zero_rotation=False) for _ in range(n_r_negative)]
        all_poses = [target_pose, *negative, *[target_pose @ r.matrix for r in r_tf]]
        labels.append(np.concatenate((np.ones(1), np.zeros(n_points - 1))))
        lt.append([Affine.from_matrix(p).translation for p in all_poses])
        lr.append([rot(p) for p in all_poses])
    gt, gr, dt, dr = [], [], [], []
    for i in batch:                                                               # get_data_grad
        trajectory = ds.trajectories[i]
        initial_index = np.random.randint(0, len(trajectory) - n_future - 1)
        required = trajectory[initial_index:initial_index + n_future + 1]
        aug_p, aug_t = [], []
        for j, pose in enumerate(required[:-1]):
            for _ in range(paf):
                a = Affine.random(t_bounds=((-0.02, 0.02),) * 3, r_bounds=((-0.6, 0.6),) * 3)
                inp, tgt = pose @ a.matrix, required[j + 1]
                if fixed_orientation is not None:
                    inp = Affine(translation=Affine.from_matrix(inp).translation, rotation=fixed_orientation).matrix
                    tgt = Affine(translation=Affine.from_matrix(tgt).translation, rotation=fixed_orientation).matrix
                aug_p.append(inp)
                aug_t.append(tgt)
        it, tt = [Affine.from_matrix(p).translation for p in aug_p], [Affine.from_matrix(p).translation for p in aug_t]
        ir, tr = [rot(p) for p in aug_p], [rot(p) for p in aug_t]
        gt.append(it)
        gr.append(ir)
        dt.append([b - a for b, a in zip(tt, it)])
        dr.append([b - a for b, a in zip(tr, ir)])
    f32 = lambda a: np.array(a, dtype=np.float32)
    return [f32(lt), f32(lr), f32(gt), f32(gr), f32(imgs), f32(ks), f32(es)], [f32(labels), f32(dt), f32(dr)]


@pytest.fixture(scope='module')
def dataset():
    return T.SyntheticLanguageDataset(n_scenes=3, n_perspectives=5, height=8, width=12, seed=3)


@pytest.mark.parametrize('representation', ['quaternion', '6d'])
@pytest.mark.parametrize('fixed_orientation', [None, [np.pi, 0.0, np.pi / 2]])
def test_generator_matches_scipy_restatement(dataset, representation, fixed_orientation):
    gen = T.LanguageDataGenerator(dataset, BOUNDS, n_views=2, batch_size=2, shuffle=False, pose_augmentation_factor=4, n_future_poses=3,
                                  fixed_orientation=fixed_orientation, rotation_representation=representation)
    for seed in (0, 1):
        np.random.seed(seed)
        (inputs, features), labels = gen[0]
        state_after = np.random.get_state()[1].copy()
        np.random.seed(seed)
        ref_inputs, ref_labels = reference_batch(dataset, gen.indices[0:2], 2, 4, 3, fixed_orientation, representation)
        assert np.array_equal(np.random.get_state()[1], state_after)             # the same number of draws
        assert inputs[7] is None
        for got, want in zip(list(inputs[:7]) + list(labels), ref_inputs + ref_labels):
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.array_equal(got, want)
        assert features.shape == (2, 2, 8, 12, 256) and features.dtype == np.float32


def test_restated_rotations_match_scipy():
    rng = np.random.default_rng(0)
    rpy = rng.uniform(-2 * np.pi, 2 * np.pi, (4000, 3))
    q = T.quat_from_euler_xyz(rpy)
    assert np.array_equal(q, Rotation.from_euler('xyz', rpy).as_quat())
    assert np.array_equal(T.matrix_from_quat(q), Rotation.from_euler('xyz', rpy).as_matrix())
    m = Rotation.from_quat(q).as_matrix()
    assert np.array_equal(T.matrix_from_quat(T.quat_normalize(q)), m)
    prod = m[:2000] @ m[2000:]                                                   # slightly off-orthogonal inputs
    assert np.array_equal(T.quat_from_matrix(prod), Rotation.from_matrix(prod).as_quat())
    axes = rng.standard_normal((3000, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    near_pi = Rotation.from_rotvec(axes * (np.pi - rng.uniform(0, 1e-5, (3000, 1)))).as_matrix()
    assert np.array_equal(T.quat_from_matrix(near_pi), Rotation.from_matrix(near_pi).as_quat())
    exact_pi = np.array([np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])])
    assert np.array_equal(T.quat_from_matrix(exact_pi), Rotation.from_matrix(exact_pi).as_quat())
    assert np.allclose(T.rotvec_from_matrix(prod), Rotation.from_matrix(prod).as_rotvec(), atol=1e-12)


def test_label_layout_and_split(dataset):
    gen = T.LanguageDataGenerator(dataset, BOUNDS, batch_size=1, pose_augmentation_factor=32, n_future_poses=6, rotation_representation='6d')
    assert (gen.n_points_train, gen.n_negative, gen.n_r_negative) == (192, 162, 24)
    fixed = T.LanguageDataGenerator(dataset, BOUNDS, pose_augmentation_factor=32, n_future_poses=6, fixed_orientation=[np.pi, 0, 0])
    assert (fixed.n_negative, fixed.n_r_negative) == (186, 0)
    np.random.seed(5)
    (inputs, _), labels = gen[0]
    assert labels[0].shape == (1, 192) and labels[0][0, 0] == 1 and not labels[0][0, 1:].any()
    target = dataset.grasp_poses[gen.indices[0]]
    assert np.array_equal(inputs[0][0, 0], target[:3, 3].astype(np.float32))
    # the last 24 are rotation negatives: within 1 cm of the target, and rotated
    t_r = inputs[0][0, 168:].astype(np.float64)
    assert np.abs(t_r - target[:3, 3]).max() <= 0.01 * math.sqrt(3) + 1e-6
    assert np.linalg.norm(t_r - target[:3, 3], axis=1).max() < np.sqrt(3) * 0.01 + 1e-6
    r6 = inputs[1][0, 168:]
    assert np.abs(r6 - np.concatenate([target[:3, 0], target[:3, 1]])).max(1).min() > 1e-5
    # the negatives in between are in the workspace
    t_n = inputs[0][0, 1:168]
    b = np.asarray(BOUNDS, dtype=np.float32)
    assert (t_n >= b[:, 0]).all() and (t_n <= b[:, 1]).all()


def test_grad_targets_are_next_pose_minus_input(dataset):
    gen = T.LanguageDataGenerator(dataset, BOUNDS, batch_size=1, pose_augmentation_factor=3, n_future_poses=4, rotation_representation='quaternion')
    np.random.seed(2)
    index = gen.indices[0]
    (inputs, _), labels = gen[0]
    np.random.seed(2)
    np.random.choice(range(5), size=1, replace=False)
    for _ in range(gen.n_negative + gen.future_poses - 1):
        T.draw_affine(BOUNDS)
    for _ in range(gen.n_r_negative):
        T.draw_affine(((-0.01, 0.01),) * 3, allow_zero_rotation=False)
    start = np.random.randint(0, len(dataset.trajectories[index]) - 4 - 1)
    nxt = dataset.trajectories[index][start + 1:start + 5]
    targets = np.repeat(nxt, 3, axis=0)
    d_t = (targets[:, :3, 3] - inputs[2][0].astype(np.float64)).astype(np.float32)
    d_r = (T.quat_from_matrix(targets[:, :3, :3]) - inputs[3][0].astype(np.float64)).astype(np.float32)
    assert np.allclose(labels[1][0], d_t, atol=1e-7)
    assert np.allclose(labels[2][0], d_r, atol=1e-7)
    # inputs are within the augmentation range of the trajectory pose they come from
    base = np.repeat(dataset.trajectories[index][start:start + 4], 3, axis=0)
    assert np.abs(inputs[2][0] - base[:, :3, 3]).max() < 0.02 * math.sqrt(3) + 1e-6


def test_dataset_shapes_and_trajectory(dataset):
    assert len(dataset) == 3
    for i in range(3):
        traj = dataset.trajectories[i]
        assert traj.shape[0] >= 3 + 2 and np.array_equal(traj[-1], dataset.grasp_poses[i])
        b = np.asarray(BOUNDS)
        t = dataset.grasp_poses[i][:3, 3]
        assert (t >= b[:, 0]).all() and (t <= b[:, 1]).all()
        assert dataset.colors[i][0].dtype == np.uint8 and dataset.colors[i][0].shape == (8, 12, 3)
        f = dataset.feature_map(i, 1)
        assert f.shape == (8, 12, 256) and f.dtype == np.float32 and np.array_equal(f, dataset.feature_map(i, 1))
    # the grasp point is visible in every view, and the feature map changes where it projects
    u, v = dataset.grasp_pixel(0, 0)
    assert 0 <= u < 12 and 0 <= v < 8
    moved = T.SyntheticLanguageDataset(n_scenes=3, n_perspectives=5, height=8, width=12, seed=3)
    moved.grasp_poses[0] = moved.grasp_poses[0].copy()
    moved.grasp_poses[0][:3, 3] += [0.1, 0.1, 0.0]
    assert not np.allclose(moved.feature_map(0, 0), dataset.feature_map(0, 0))


def test_get_inputs_views(dataset):
    for n_images, views in ((3, [0, 1, 2]), (2, [3, 4])):
        input_data, features, task_info, grasp = T.get_inputs(dataset, 1, n_images)
        assert input_data[0].shape == (1, n_images, 8, 12, 3) and input_data[3] is None
        assert np.array_equal(input_data[0][0, 0], (dataset.colors[1][views[0]] / 255.0).astype(np.float32))
        assert np.array_equal(input_data[2][0, -1], np.linalg.inv(dataset.cameras[1][views[-1]]['pose']).astype(np.float32))
        assert np.array_equal(features[0, 0], dataset.feature_map(1, views[0]))
        assert task_info is dataset.task_info[1] and grasp is dataset.grasp_poses[1]
    with pytest.raises(ValueError):
        T.get_inputs(dataset, 0, 1)


def test_grasp_error_closed_forms():
    a = T.affine_from_euler([0.4, -0.1, 0.05], [0.3, -1.2, 2.0])
    b = a.copy()
    b[:3, 3] += [0.003, -0.004, 0.0]
    t, r = T.grasp_error(a, b)
    assert abs(t - 0.005) < 1e-12 and r < 1e-7
    for theta in (1e-4, 0.3, 1.7, 3.0):
        axis = np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5])
        c = a.copy()
        c[:3, :3] = a[:3, :3] @ Rotation.from_rotvec(theta * axis).as_matrix()
        t, r = T.grasp_error(a, c)
        assert t == 0.0 and abs(r - theta) < 1e-9


def test_get_step_results_order():
    losses_r = np.array([0.5, 0.9, 0.1, 0.7, 0.95, 0.3, 0.8])
    poses = np.tile(np.eye(4), (7, 1, 1))
    poses[:, 0, 3] = np.arange(7) * 0.001
    res = T.get_step_results(losses_r * 0, losses_r, poses, poses, np.eye(4))
    assert [float(s) for s in res['final_success']] == [0.5, 0.7, 0.8, 0.9, 0.95]          # ascending: the best last
    assert [round(e[0] * 1000) for e in res['errors_r']] == [0, 3, 6, 1, 4]
    assert res['errors_r'][-1] == T.grasp_error(np.eye(4), poses[4])


def test_log_results_units():
    results = [{'errors_r': [(0.002, np.pi / 180), (0.004, 3 * np.pi / 180)]}, {'errors_r': [(0.006, 0.0), (0.010, np.pi / 18)]}]
    got = []
    d = T.log_results(7, results, log=got.append, print_fn=lambda *_: None)
    assert got == [d] and d['epoch'] == 7
    assert abs(d['mean_r_error_t'] - 5.5) < 1e-12 and abs(d['mean_r_error_r'] - 3.5) < 1e-12
    assert abs(d['best_r_error_mean_t'] - 7.0) < 1e-12 and abs(d['best_r_error_mean_r'] - 6.5) < 1e-12


def test_load_training_progress(tmp_path):
    best, n_fits, start, start_fit, path = T.load_training_progress(4, str(tmp_path), 400)
    assert (best, n_fits, start, start_fit) == ([2000, 2000], 100, 0, 0)
    with open(path, 'w') as f:
        json.dump({'epoch': 12, 'best_mean_error': [0.01, 0.2]}, f)
    best, n_fits, start, start_fit, _ = T.load_training_progress(4, str(tmp_path), 400)
    assert (best, n_fits, start, start_fit) == ([0.01, 0.2], 100, 12, 3)


def test_best_model_rule():
    assert T.combined_error([0.002, np.pi / 180]) == pytest.approx(3.0)
    assert T.combined_error([0.004, 0.0]) < T.combined_error([2000, 2000])
    # 1 mm is worth 1 degree: 3 mm + 1 deg beats 1 mm + 4 deg
    assert T.combined_error([0.003, np.pi / 180]) < T.combined_error([0.001, 4 * np.pi / 180])


def test_load_grasp_readout_keras_order():
    torch.manual_seed(0)
    ro = GraspReadout(42, use_bias=True)
    rng = np.random.default_rng(1)
    shapes = [(128, 64), (64,)] * 4 + [(256, 64), (64,)] + [(2688, 128), (128,), (128, 64), (64,), (2688, 64)] + \
             [(64, 64), (64,), (64, 64), (64,)] + [(64, 1), (1,)]
    arrays = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    weight_before = ro.block_0.layer_0.weight
    load_grasp_readout(ro, arrays)
    assert ro.block_0.layer_0.weight is weight_before                            # in place
    assert np.array_equal(ro.activation_downscale[2].weight.detach().numpy(), arrays[4].T)
    assert np.array_equal(ro.combined_activation_downscale.bias.detach().numpy(), arrays[9])
    assert np.array_equal(ro.block_0.layer_1.weight.detach().numpy(), arrays[12].T)
    assert np.array_equal(ro.block_0.shortcut.weight.detach().numpy(), arrays[14].T)
    assert np.array_equal(ro.block_1.layer_1.bias.detach().numpy(), arrays[18])
    assert np.array_equal(ro.output_layer.weight.detach().numpy(), arrays[19].T)
    assert np.array_equal(ro.output_layer.bias.detach().numpy(), arrays[20])
    with pytest.raises(ValueError):
        load_grasp_readout(ro, arrays[:-1])


def test_categorical_crossentropy_from_logits():
    logits = torch.tensor([[2.0, 0.5, -1.0], [0.1, 0.2, 0.3]], dtype=torch.float64)
    labels = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    p = np.exp(logits.numpy()) / np.exp(logits.numpy()).sum(1, keepdims=True)
    want = -(np.log(p[0, 0]) + np.log(p[1, 2])) / 2
    assert abs(float(categorical_crossentropy_from_logits(labels, logits)) - want) < 1e-12


def test_select_loss():
    assert T.select_loss('kl_divergence')[1] is True
    assert T.select_loss('cross_entropy') == (categorical_crossentropy_from_logits, False)
    with pytest.raises(ValueError):
        T.select_loss('mse')
