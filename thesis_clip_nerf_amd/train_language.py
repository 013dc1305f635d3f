"""`train_language.py`-shaped grasp-model training loop on the HIP trunk (reference: src/train_language.py, utils/training.py:23-78,
utils/optimization.py:11-37,108-133, utils/util.py:19-114, data_generator/language.py + base.py).

Same structure and names as the reference - `LanguageDataGenerator`, `get_inputs`, `validate`, `get_step_results`, `log_results`,
`load_training_progress`, `train_grasp_model` - with what is not in this repository's scope replaced by explicit stand-ins:

* the dataset submodule (`load_dataset_language`, absent from the reference tree) -> :class:`SyntheticLanguageDataset`;
* the frozen encoders (CLIP + visual features) -> a per-view feature map supplied by the dataset, since `combined_features` is an
  input of the hot path.  By default that is the synthetic bump map and `inputs[7]` (the CLIP tokens) is None; with
  :class:`EncodedLanguageDataset` (`--encoder v4`) the map comes from `encoders.LanguageFeatureProducer` - the reference's
  CombineCLIPVisualV4 on stand-ins for CLIP - run on the view and on the tokens of the scene's instruction, and `with_tokens=True`
  puts those tokens, int32 (B, 77), into `inputs[7]`;
* `OracleAgent.calculate_error` (src/lib/agents, absent) -> :func:`grasp_error`, the vendored `transformation_difference`;
* `manipulation_tasks.Affine` / scipy `Rotation` -> the NumPy restatements below, with scipy's operation order;
* hydra -> argparse; wandb -> a callback; loguru -> `log`.

    python -m thesis_clip_nerf_amd.train_language --model-path /tmp/language_run --backbone-path /tmp/mvnerf_run --init-backbone
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
import time

import numpy as np
import torch

from ._lib import NET_PARAMS
from .grasp_optimizer import DEFAULT_WORKSPACE_BOUNDS, DNGFOptimizer, compute_results
from .lmvnerf import LanguageNeRF, categorical_crossentropy_from_logits, kl_divergence, store_trunk
from .encoders import tokenize
from .model import camera_parameters
from .synthetic import glorot_net, pinhole, ring_pose
from .train_nerf import init_training_session


# ---- scipy.spatial.transform.Rotation, restated (the order of every operation as scipy 1.x computes it) -------------------------------
def _compose_quat(p, q):
    """Rotation p * q on (..., 4) quaternions (x, y, z, w): scipy's `_compose_quat`."""
    c0 = p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1]
    c1 = p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2]
    c2 = p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]
    return np.stack([p[..., 3] * q[..., 0] + q[..., 3] * p[..., 0] + c0,
                     p[..., 3] * q[..., 1] + q[..., 3] * p[..., 1] + c1,
                     p[..., 3] * q[..., 2] + q[..., 3] * p[..., 2] + c2,
                     p[..., 3] * q[..., 3] - p[..., 0] * q[..., 0] - p[..., 1] * q[..., 1] - p[..., 2] * q[..., 2]], -1)


def quat_from_euler_xyz(rpy):
    """Rotation.from_euler('xyz', rpy).as_quat(): extrinsic x, y, z as a composition of elementary quaternions (not renormalised)."""
    rpy = np.asarray(rpy, dtype=np.float64)

    def elementary(axis, angle):
        q = np.zeros(angle.shape + (4,))
        q[..., 3] = np.cos(angle / 2)
        q[..., axis] = np.sin(angle / 2)
        return q
    q = elementary(0, rpy[..., 0])
    for axis in (1, 2):
        q = _compose_quat(elementary(axis, rpy[..., axis]), q)
    return q


def quat_normalize(q):
    """Rotation.from_quat(q) stores q / |q|."""
    n = np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3])
    return q / n[..., None]


def matrix_from_quat(q):
    """Rotation.as_matrix() of a stored quaternion q (x, y, z, w), (..., 4) -> (..., 3, 3)."""
    x, y, z, w = (q[..., i] for i in range(4))
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    m = np.stack([x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw),
                  2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw),
                  2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def quat_from_matrix(m):
    """Rotation.from_matrix(m).as_quat(), (..., 3, 3) -> (..., 4): the case picked by the largest of (m00, m11, m22, trace) (the first on
    ties), the sign that case gives (not made canonical), then normalised."""
    m = np.asarray(m, dtype=np.float64)
    shape = m.shape[:-2]
    m = m.reshape(-1, 3, 3)
    q = np.empty((m.shape[0], 4))
    decision = np.stack([m[:, 0, 0], m[:, 1, 1], m[:, 2, 2], m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]], -1)
    choice = np.argmax(decision, -1)
    for c in range(3):
        s = choice == c
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[s, i] = 1 - decision[s, 3] + 2 * m[s, i, i]
        q[s, j] = m[s, j, i] + m[s, i, j]
        q[s, k] = m[s, k, i] + m[s, i, k]
        q[s, 3] = m[s, k, j] - m[s, j, k]
    s = choice == 3
    q[s, 0] = m[s, 2, 1] - m[s, 1, 2]
    q[s, 1] = m[s, 0, 2] - m[s, 2, 0]
    q[s, 2] = m[s, 1, 0] - m[s, 0, 1]
    q[s, 3] = 1 + decision[s, 3]
    return quat_normalize(q).reshape(shape + (4,))


def rotvec_from_matrix(m):
    """Rotation.from_matrix(m).as_rotvec() (the angle in [0, pi]), (..., 3, 3) -> (..., 3)."""
    q = quat_from_matrix(m)
    q = np.where(q[..., 3:] < 0, -q, q)
    xyz = q[..., :3]
    angle = 2 * np.arctan2(np.sqrt((xyz * xyz).sum(-1)), q[..., 3])
    a2 = angle * angle
    with np.errstate(divide='ignore', invalid='ignore'):
        scale = np.where(angle <= 1e-3, 2 + a2 / 12 + 7 * a2 * a2 / 2880, angle / np.sin(angle / 2))
    return scale[..., None] * xyz


# ---- manipulation_tasks.transform.Affine, as the generator uses it ---------------------------------------------------------------------
def draw_affine(t_bounds=((0, 1), (0, 1), (0, 1)), r_bounds=((0, 2 * np.pi), (0, 2 * np.pi), (0, 2 * np.pi)), allow_zero_rotation=True):
    """The draws of Affine.random (transform.py:32-55) from numpy's global RNG, in its order: t ~ U(t_bounds), then rpy ~ U(r_bounds),
    redrawn while every angle is < 1e-4 when allow_zero_rotation=False -> (t, rpy)."""
    t_b = np.array(t_bounds)
    translation = np.random.uniform(t_b[:, 0], t_b[:, 1])
    r_b = np.array(r_bounds)
    if not allow_zero_rotation:
        rpy = np.array([0.0, 0.0, 0.0])
        while (rpy < 0.0001).all():
            rpy = np.random.uniform(r_b[:, 0], r_b[:, 1])
    else:
        rpy = np.random.uniform(r_b[:, 0], r_b[:, 1])
    return translation, rpy


def draw_affines(n, t_bounds, r_bounds=((0, 2 * np.pi), (0, 2 * np.pi), (0, 2 * np.pi))):
    """n consecutive draw_affine(t_bounds, r_bounds) (allow_zero_rotation=True) as one (n, 6) draw: numpy's legacy uniform fills it in
    C order with low + (high - low) * u, so the values and the stream position are those of the n calls -> (t (n, 3), rpy (n, 3))."""
    t_b, r_b = np.array(t_bounds, dtype=np.float64), np.array(r_bounds, dtype=np.float64)
    d = np.random.uniform(np.concatenate([t_b[:, 0], r_b[:, 0]]), np.concatenate([t_b[:, 1], r_b[:, 1]]), size=(n, 6))
    return d[:, :3], d[:, 3:]


def affines_from_draws(translations, rpys):
    """Affine.random's matrices from its draws, (n, 3), (n, 3) -> (n, 4, 4): the rotation made as the reference makes it, from_euler ->
    as_quat -> Affine(rotation=quat) -> from_quat (normalised) -> as_matrix (element-wise, so batching changes no bit)."""
    translations, rpys = np.asarray(translations, dtype=np.float64).reshape(-1, 3), np.asarray(rpys, dtype=np.float64).reshape(-1, 3)
    m = np.tile(np.eye(4), (translations.shape[0], 1, 1))
    m[:, :3, 3] = translations
    m[:, :3, :3] = matrix_from_quat(quat_normalize(quat_from_euler_xyz(rpys)))
    return m


def affine_from_euler(translation, rpy):
    """Affine(translation=t, rotation=rpy).matrix for a 3-element rpy: from_euler('xyz').as_matrix() (the quaternion as composed)."""
    m = np.eye(4)
    m[:3, 3] = np.array(translation)
    m[:3, :3] = matrix_from_quat(quat_from_euler_xyz(rpy))
    return m


def pose_rotation(poses, rotation_representation):
    """Affine.from_matrix(pose).quat, or [rotation[:, 0], rotation[:, 1]] for '6d', of (n, 4, 4) poses -> (n, 4 | 6) float64."""
    poses = np.asarray(poses, dtype=np.float64)
    if rotation_representation == 'quaternion':
        return quat_from_matrix(poses[:, :3, :3])
    if rotation_representation == '6d':
        return np.concatenate([poses[:, :3, 0], poses[:, :3, 1]], -1)
    raise ValueError('Unknown rotation representation: ' + str(rotation_representation))


# ---- data ------------------------------------------------------------------------------------------------------------------------------
class SyntheticLanguageDataset:
    """Stand-in for `load_dataset_language(n_perspectives, path)`: per scene `n_perspectives` uint8 views on a ring around the workspace
    (camera configs as the dataset stores them: 'pose' camera-to-world, 'intrinsics' (9,)), a grasp pose inside the workspace bounds, a
    trajectory of `trajectory_length` poses that ends at it, and a per-view (H, W, 256) float32 feature map - the frozen encoders'
    stand-in - with a bump where the grasp point projects, so the map says where to grasp.  Feature maps are computed on demand
    (:meth:`feature_map`, deterministic): at 480 x 640 one is 315 MB."""

    def __init__(self, n_scenes=4, n_perspectives=5, height=32, width=32, workspace_bounds=DEFAULT_WORKSPACE_BOUNDS, trajectory_length=10,
                 seed=0):
        rng = np.random.default_rng(seed)
        b = np.asarray(workspace_bounds, dtype=np.float64)
        self.n_perspectives, self.height, self.width = n_perspectives, height, width
        self.k = pinhole(width, height)
        self.centre = b.mean(1)
        self.proj = rng.standard_normal((3, 256)).astype(np.float32)
        self.grasp_direction = rng.standard_normal(256).astype(np.float32)
        self.colors, self.cameras, self.grasp_poses, self.trajectories, self.task_info = [], [], [], [], []
        inner = b.mean(1, keepdims=True) + 0.8 * (b - b.mean(1, keepdims=True))
        for i in range(n_scenes):
            base = rng.random((height, width, 3))
            cols, cams = [], []
            for p in range(n_perspectives):
                img = np.clip(base + 0.05 * rng.standard_normal(base.shape), 0, 1)
                cols.append((img * 255).astype(np.uint8))
                cams.append({'pose': ring_pose(2 * np.pi * p / n_perspectives + rng.uniform(-0.1, 0.1), centre=self.centre),
                             'intrinsics': self.k.reshape(-1).copy()})
            grasp = affine_from_euler(rng.uniform(inner[:, 0], inner[:, 1]), [np.pi, 0.0, rng.uniform(0, 2 * np.pi)])  # top-down, any yaw
            n = trajectory_length
            traj = [grasp @ affine_from_euler([0.0, 0.0, -0.15 * (1 - s)], [0.0, 0.0, 0.5 * (1 - s)]) for s in np.arange(n) / (n - 1)]
            traj[-1] = grasp.copy()
            self.colors.append(cols)
            self.cameras.append(cams)
            self.grasp_poses.append(grasp)
            self.trajectories.append(np.array(traj))
            self.task_info.append({f'object_{j}': {'id': j} for j in range(1 + i % 3)})

    def __len__(self):
        return len(self.colors)

    def grasp_pixel(self, i, p):
        """(u, v) of scene i's grasp point in view p."""
        cam = self.cameras[i][p]
        x = np.linalg.inv(cam['pose']) @ np.append(self.grasp_poses[i][:3, 3], 1.0)
        uvw = self.k.astype(np.float64) @ x[:3]
        return uvw[0] / uvw[2], uvw[1] / uvw[2]

    def feature_map(self, i, p):
        """tanh(colour projection + 3 * bump(grasp pixel) * direction), (H, W, 256) float32."""
        u, v = self.grasp_pixel(i, p)
        sigma = 0.08 * min(self.height, self.width)
        yy, xx = np.mgrid[0:self.height, 0:self.width]
        bump = np.exp(-((xx - u) ** 2 + (yy - v) ** 2) / (2 * sigma * sigma)).astype(np.float32)
        img = self.colors[i][p].astype(np.float32) / np.float32(255)
        return np.tanh((img * 2 - 1) @ self.proj + (3 * bump)[..., None] * self.grasp_direction)

    OBJECT_NAMES = ('red block', 'green bowl', 'blue mug')

    def instruction(self, i):
        """The scene's instruction, from its task_info: which of its objects to pick."""
        objects = sorted(self.task_info[i])
        target = self.task_info[i][objects[i % len(objects)]]['id']
        return f'pick up the {self.OBJECT_NAMES[target % len(self.OBJECT_NAMES)]}, object {target + 1} of {len(objects)}'


class EncodedLanguageDataset:
    """A language dataset whose feature maps come from the frozen encoders: every attribute of `dataset`, plus `tokens(i)` - the
    scene's instruction as int32 (77,) - and `feature_map(i, p)` = `producer` (encoders.LanguageFeatureProducer, already on the
    device it is to run on) on view p with scene i's tokens.  device=None: the map as a float32 NumPy array (the host path of the
    generator); a device: a tensor there in the producer's out_dtype, which `LanguageDataGenerator(device=...)` keeps without a host
    round trip."""

    def __init__(self, dataset, producer, device=None):
        self.dataset, self.producer = dataset, producer
        self.device = torch.device(device) if device is not None else None

    def __getattr__(self, name):                     # (only reached for what this object does not have itself)
        if name in ('dataset', 'producer', 'device'):
            raise AttributeError(name)
        return getattr(self.dataset, name)

    def __len__(self):
        return len(self.dataset)

    def tokens(self, i):
        return tokenize([self.dataset.instruction(i)])[0]

    def feature_map(self, i, p, instruction=None):
        """instruction: another text than the scene's own (what would the map be had the user asked for something else?)."""
        where = next(self.producer.parameters()).device
        image = torch.from_numpy((self.dataset.colors[i][p][..., :3] / 255.0).astype(np.float32)).to(where)
        tokens = self.tokens(i) if instruction is None else tokenize([instruction])[0]
        out = self.producer(image[None], tokens=torch.from_numpy(tokens[None]).to(where))[0]
        return out.float().cpu().numpy() if self.device is None else out.to(self.device)


class LanguageDataGenerator:
    """data_generator/language.py + base.py: keras-Sequence semantics, numpy's global RNG drawn in the reference's order (per batch:
    np.random.choice of views per scene; Affine.random for the negatives and the rotation negatives per scene; np.random.randint and the
    augmentations per scene).  `batch` -> ((inputs, features), [landscape labels, d_t, d_r]) with inputs = [translations, rotations of
    the landscape poses, translations, rotations of the gradient poses, images, intrinsics, extrinsics_inv, CLIP tokens]: what
    `LanguageNeRF.train_step(data, combined_features)` takes.  The tokens are None unless with_tokens is set: then `dataset.tokens(i)`
    of the batch, int32 (B, 77) (the feature maps of an :class:`EncodedLanguageDataset` already carry the instruction; the model
    reads `inputs[:7]`).

    device: keep every view used (image, feature map, cameras) resident on that GPU after its first use and assemble the batch there;
    only the pose arrays (a few KB) cross PCIe per step.  The batches are bit-identical to the host path's (NumPy float32 arrays)."""

    def __init__(self, dataset, workspace_bounds, n_views=1, batch_size=1, shuffle=True, pose_augmentation_factor=1, n_future_poses=5,
                 fixed_orientation=None, rotation_representation='quaternion', device=None, with_tokens=False):
        if rotation_representation not in ('quaternion', '6d'):
            raise ValueError('Unknown rotation representation: ' + rotation_representation)
        self.future_poses = n_future_poses
        self.pose_augmentation_factor = pose_augmentation_factor
        self.dataset = dataset
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.indices = np.arange(len(dataset))
        self.on_epoch_end()
        self.workspace_bounds = workspace_bounds
        self.n_views = n_views
        self.n_perspectives = dataset.n_perspectives
        self.fixed_orientation = fixed_orientation
        self.rotation_representation = rotation_representation
        self.device = torch.device(device) if device is not None else None
        self._resident = {}
        self.with_tokens = with_tokens
        self.n_points_train = self.future_poses * self.pose_augmentation_factor
        if self.fixed_orientation is not None:
            self.n_negative = self.n_points_train - self.future_poses
            self.n_r_negative = 0
        else:
            n_r_fraction = 8
            self.n_negative = ((n_r_fraction - 1) * self.n_points_train) // n_r_fraction - self.future_poses
            self.n_r_negative = self.n_points_train - self.n_negative - self.future_poses

    def on_epoch_end(self):
        if self.shuffle:
            np.random.shuffle(self.indices)

    def __len__(self):
        return len(self.indices) // self.batch_size

    def __getitem__(self, index):
        return self.get_data(self.indices[index * self.batch_size:(index + 1) * self.batch_size])

    def get_view_indices(self, batch):
        """get_data_camera's draws (language.py:38-40)."""
        return [np.random.choice(range(self.n_perspectives), size=self.n_views, replace=False) for _ in batch]

    def get_data_camera(self, batch, view_indices):
        """language.py:36-64 + the views' feature maps: images (B, V, H, W, 3) in [0, 1], intrinsics, extrinsics_inv (B, V, 4, 4),
        features (B, V, H, W, 256), all float32 NumPy."""
        ds = self.dataset
        imgs, ks, es, feats = [], [], [], []
        for i, src in zip(batch, view_indices):
            cams = [camera_parameters(ds.cameras[i][s]) for s in src]
            imgs.append([ds.colors[i][s][..., :3] / 255.0 for s in src])
            es.append([c[0] for c in cams])
            ks.append([c[1] for c in cams])
            feats.append([ds.feature_map(i, s) for s in src])
        f32 = lambda a: np.array(a, dtype=np.float32)
        return f32(imgs), f32(ks), f32(es), f32(feats)

    def _view(self, i, p):
        """Device-resident (image (H, W, 3), features (H, W, 256), extrinsics_inv, intrinsics) of scene i, perspective p."""
        key = (int(i), int(p))
        if key not in self._resident:
            ds, dev = self.dataset, self.device
            einv, k4 = camera_parameters(ds.cameras[i][p])
            host = ((ds.colors[i][p][..., :3] / 255.0).astype(np.float32), ds.feature_map(i, p), einv.astype(np.float32), k4.astype(np.float32))
            self._resident[key] = tuple(a.to(dev) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                                        for a in host)
        return self._resident[key]

    def get_data_camera_device(self, batch, view_indices):
        """get_data_camera with the batch gathered from the resident views on the device: (images, intrinsics, extrinsics_inv, features)."""
        views = [[self._view(i, s) for s in src] for i, src in zip(batch, view_indices)]
        return tuple(torch.stack([torch.stack([v[k] for v in scene]) for scene in views]) for k in (0, 3, 2, 1))

    def get_data_landscape_final(self, batch):
        """language.py:66-103: the target pose (label 1), n_negative + future_poses - 1 poses anywhere in the workspace and n_r_negative
        poses within 1 cm and a non-zero rotation of the target (labels 0)."""
        input_translations, input_rotations, targets = [], [], []
        for i in batch:
            target_pose = self.dataset.grasp_poses[i]
            negative_samples = affines_from_draws(*draw_affines(self.n_negative + self.future_poses - 1, self.workspace_bounds))
            draws = [draw_affine(t_bounds=((-0.01, 0.01), (-0.01, 0.01), (-0.01, 0.01)), allow_zero_rotation=False)
                     for _ in range(self.n_r_negative)]
            negative_r_samples = [target_pose @ r for r in affines_from_draws(*zip(*draws))] if draws else []
            all_poses = np.array([target_pose, *negative_samples, *negative_r_samples])
            targets.append(np.concatenate((np.ones(1), np.zeros(self.n_points_train - 1)), axis=0))
            input_translations.append(all_poses[:, :3, 3])
            input_rotations.append(pose_rotation(all_poses, self.rotation_representation))
        return (np.array(input_translations, dtype=np.float32), np.array(input_rotations, dtype=np.float32),
                np.array(targets, dtype=np.float32))

    def get_data_grad(self, batch):
        """language.py:105-167: future_poses consecutive trajectory poses, each augmented pose_augmentation_factor times (+-2 cm,
        +-0.6 rad); targets are the next trajectory pose minus the input (translation and rotation representation)."""
        translations, rotations, target_d_t, target_d_q = [], [], [], []
        for i in batch:
            trajectory = self.dataset.trajectories[i]
            initial_index = np.random.randint(0, len(trajectory) - self.future_poses - 1)
            required_poses = trajectory[initial_index:initial_index + self.future_poses + 1]
            paf = self.pose_augmentation_factor
            augmentations = affines_from_draws(*draw_affines(self.future_poses * paf, ((-0.02, 0.02), (-0.02, 0.02), (-0.02, 0.02)),
                                                             ((-0.6, 0.6), (-0.6, 0.6), (-0.6, 0.6))))
            inp = np.array([required_poses[n // paf] @ a for n, a in enumerate(augmentations)])       # pose j, augmentation n % paf
            tgt = np.repeat(required_poses[1:], paf, axis=0)
            if self.fixed_orientation is not None:
                inp = np.array([affine_from_euler(p[:3, 3], self.fixed_orientation) for p in inp])
                tgt = np.array([affine_from_euler(p[:3, 3], self.fixed_orientation) for p in tgt])
            input_rotations = pose_rotation(inp, self.rotation_representation)
            translations.append(inp[:, :3, 3])
            rotations.append(input_rotations)
            target_d_t.append(tgt[:, :3, 3] - inp[:, :3, 3])
            target_d_q.append(pose_rotation(tgt, self.rotation_representation) - input_rotations)
        f32 = lambda a: np.array(a, dtype=np.float32)
        return f32(translations), f32(rotations), f32(target_d_t), f32(target_d_q)

    def get_data(self, batch):
        view_indices = self.get_view_indices(batch)
        landscape = self.get_data_landscape_final(batch)
        grad = self.get_data_grad(batch)
        if self.device is not None:
            images, intrinsics, extrinsics_inv, features = self.get_data_camera_device(batch, view_indices)
            landscape, grad = ([torch.from_numpy(a).to(self.device) for a in arrays] for arrays in (landscape, grad))
        else:
            images, intrinsics, extrinsics_inv, features = self.get_data_camera(batch, view_indices)
        tokens = None
        if self.with_tokens:
            tokens = np.stack([self.dataset.tokens(i) for i in batch]).astype(np.int32)
            if self.device is not None:
                tokens = torch.from_numpy(tokens).to(self.device)
        inputs = [landscape[0], landscape[1], grad[0], grad[1], images, intrinsics, extrinsics_inv, tokens]
        return (inputs, features), [landscape[2], grad[2], grad[3]]


def get_inputs(dataset, sample_idx, n_images, device=None, with_tokens=False):
    """utils/util.py:74-114: views 0-2 for n_images = 3, views 3-4 for n_images = 2 -> (input_data [images (1, n, H, W, 3),
    intrinsics, extrinsics_inv (1, n, 4, 4), tokens (None, or int32 (1, 77) with with_tokens)], features (1, n, H, W, 256), task_info,
    grasp_pose (4, 4)).  device: the arrays as float32 tensors there (copied once; the validation passes then read them in place)."""
    if n_images == 2:
        views = range(3, 5)
    elif n_images == 3:
        views = range(0, 3)
    else:
        raise ValueError(f'n_images = {n_images}: the reference selects views for 2 or 3 images only')
    cams = [camera_parameters(dataset.cameras[sample_idx][i]) for i in views]
    observations = np.array([[dataset.colors[sample_idx][i][..., :3] / 255.0 for i in views]], dtype=np.float32)
    intrinsics = np.array([[c[1] for c in cams]], dtype=np.float32)
    extrinsics_inv = np.array([[c[0] for c in cams]], dtype=np.float32)
    maps = [dataset.feature_map(sample_idx, i) for i in views]
    tokens = dataset.tokens(sample_idx)[None].astype(np.int32) if with_tokens else None
    input_data = [observations, intrinsics, extrinsics_inv]
    if device is not None:
        input_data = [torch.from_numpy(a).to(device) for a in input_data]
        if isinstance(maps[0], torch.Tensor):                                # an encoded dataset on a device: no host round trip
            features = torch.stack([m.to(device=device, dtype=torch.float32) for m in maps])[None]
        else:
            features = torch.from_numpy(np.array([maps], dtype=np.float32)).to(device)
        tokens = torch.from_numpy(tokens).to(device) if with_tokens else None
    else:
        features = np.array([maps], dtype=np.float32)
    return input_data + [tokens], features, dataset.task_info[sample_idx], dataset.grasp_poses[sample_idx]


# ---- validation (utils/optimization.py, utils/util.py) -----------------------------------------------------------------------------------
def grasp_error(gt_h, pose_h):
    """(translation error [m], rotation error [rad]) between two 4 x 4 poses: transformation_difference (transform_utils/differences.py:
    55-58), |t_a - t_b| and |axis_angle(A^-1 B)|.  Stand-in for `OracleAgent.calculate_error` (src/lib/agents is absent)."""
    a, b = np.asarray(gt_h, dtype=np.float64), np.asarray(pose_h, dtype=np.float64)
    t_err = float(np.linalg.norm(a[:3, 3] - b[:3, 3]))
    r_err = float(np.linalg.norm(rotvec_from_matrix((np.linalg.inv(a) @ b)[:3, :3])))
    return t_err, r_err


def get_step_results(losses_t, losses_r, trajectory_t, trajectory_r, gt_grasp_pose_h):
    """optimization.py:108-133: the five poses of highest final success (rotation phase), in ascending order of success, and their
    errors to the ground truth: errors_r[-1] belongs to the best."""
    best_grasp_indices_r = np.argsort(losses_r)[-5:]
    best_grasp_poses_r = [trajectory_r[k] for k in best_grasp_indices_r]
    final_success_r = [losses_r[k] for k in best_grasp_indices_r]
    errors_r = [grasp_error(gt_grasp_pose_h, pose) for pose in best_grasp_poses_r]
    return {'grasp_poses': best_grasp_poses_r, 'final_success': final_success_r, 'errors_r': errors_r}


def validate(pose_optimizer, optimization_config, valid_data, log=print):
    """optimization.py:11-37: compute_results on every validation sample -> the list of get_step_results."""
    results = []
    for i, (input_data, features, task_info, grasp_pose_h) in enumerate(valid_data):
        log(f'Validating on sample {i + 1} with {len(task_info.keys())} objects ...')
        losses_t, losses_r, grasps_t, grasps_r, _, _ = compute_results(pose_optimizer, input_data, features, False, **optimization_config)
        result = get_step_results(losses_t, losses_r, grasps_t, grasps_r, grasp_pose_h)
        results.append(result)
        best = result['errors_r'][-1]
        log(f'   Best    {best[0] * 1000}    {best[1] / np.pi * 180}')
    return results


def log_results(epoch, results, log=None, print_fn=print):
    """util.py:48-71: mean error over all five poses and over the best ones, in mm and degrees -> the dict, also passed to `log` (the
    wandb.log stand-in) when given."""
    r_errors = [r['errors_r'] for r in results]
    mean_r_error = np.mean(np.concatenate(r_errors, axis=0), axis=0)
    best_r_error_mean = np.mean(np.stack([errors_r[-1] for errors_r in r_errors], axis=0), axis=0)
    log_dict = {'epoch': epoch,
                'mean_r_error_t': mean_r_error[0] * 1000, 'mean_r_error_r': mean_r_error[1] / np.pi * 180,
                'best_r_error_mean_t': best_r_error_mean[0] * 1000, 'best_r_error_mean_r': best_r_error_mean[1] / np.pi * 180}
    print_fn(f"   Average   {log_dict['mean_r_error_t']}    {log_dict['mean_r_error_r']}")
    print_fn(f"   Best   {log_dict['best_r_error_mean_t']}    {log_dict['best_r_error_mean_r']}")
    if log is not None:
        log(log_dict)
    return log_dict


def read_best_mean_error(training_progress_file):
    """util.py:40-48: [2000, 2000] unless training_progress.json holds one."""
    best_mean_error = [2000, 2000]
    if os.path.exists(training_progress_file):
        with open(training_progress_file) as f:
            best_mean_error = json.load(f).get('best_mean_error', best_mean_error)
    return best_mean_error


def load_training_progress(eval_after_epochs, model_log_dir, n_epochs):
    """util.py:19-24 -> (best_mean_error, n_fits, start_epoch, start_n_fit, training_progress_file)."""
    start_epoch, training_progress_file = init_training_session(model_log_dir)
    best_mean_error = read_best_mean_error(training_progress_file)
    return best_mean_error, n_epochs // eval_after_epochs, start_epoch, start_epoch // eval_after_epochs, training_progress_file


def combined_error(mean_error):
    """The model-selection score of training.py:59: t [m] * 1000 + r [rad] / pi * 180."""
    return mean_error[0] * 1000 + mean_error[1] / np.pi * 180


# ---- training ----------------------------------------------------------------------------------------------------------------------------
def fit(grasp_model, data_generator, epochs, initial_epoch=0, log=print):
    """Keras `Model.fit(generator, epochs=, initial_epoch=)` over LanguageNeRF.train_step, `on_epoch_end` after each epoch -> one dict of
    epoch means per epoch ('loss' = landscape + both gradient losses)."""
    history = []
    for epoch in range(initial_epoch, epochs):
        outs = []
        for step in range(len(data_generator)):
            (inputs, features), labels = data_generator[step]
            outs.append(grasp_model.train_step((inputs, labels), features))
        data_generator.on_epoch_end()
        means = {k: float(torch.stack([o[k].reshape(()) for o in outs]).mean()) if outs else float('nan')
                 for k in ('landscape_loss', 'grad_loss_t', 'grad_loss_r', 'pred')}
        means['loss'] = means['landscape_loss'] + means['grad_loss_t'] + means['grad_loss_r']
        history.append(means)
        log(f'Epoch {epoch + 1}/{epochs} - ' + ' - '.join(f'{k}: {v:.6f}' for k, v in means.items()))
    return history


def train_grasp_model(grasp_model, data_generator, n_epochs, eval_after_epochs, model_log_dir, model_checkpoint_name, grasp_optimizer,
                      optimization_config, callback, valid_data, log=print, fused_tail=False, fused_step=False, fused_optimizer=False):
    """training.py:23-78 (`callback` takes the place of wandb_config: called with log_results' dict).  One validation on valid_data[:1]
    first, as the reference does (also on a resumed run); then per `eval_after_epochs`: fit, validate all, results-{e}.pkl, log, store
    `{model_log_dir}/best` on a better t*1000 + r/pi*180, training_progress.json, the checkpoint.  -> the fit history.
    fused_tail: the read-out's per-pose layers as fused HIP passes for this run (LanguageNeRF.set_fused_tail; the default is today's
    layer-by-layer path).  fused_step: the training step up to the optimiser as one C call for this run (LanguageNeRF.set_fused_step).
    fused_optimizer: the optimiser inside that call too (LanguageNeRF.set_fused_optimizer: Keras Adam with a device-side step counter;
    implies fused_step).  Its moments are in no checkpoint, as torch's are not: a resumed run starts them at zero either way."""
    fused_step = bool(fused_step or fused_optimizer)
    if fused_tail or getattr(getattr(grasp_model, 'grasp_readout', None), 'fused_tail', False):
        grasp_model.set_fused_tail(bool(fused_tail))
    if not fused_optimizer and getattr(grasp_model, 'fused_optimizer', False):
        grasp_model.set_fused_optimizer(False)
    if fused_step or getattr(grasp_model, 'fused_step', False):
        grasp_model.set_fused_step(fused_step)
    if fused_optimizer:
        grasp_model.set_fused_optimizer(True)
    best_mean_error, n_fits, start_epoch, start_n_fit, training_progress_file = load_training_progress(eval_after_epochs, model_log_dir,
                                                                                                       n_epochs)
    log(f'Starting training from epoch {start_epoch}; best mean error {best_mean_error}')
    os.makedirs(f'{model_log_dir}/valid', exist_ok=True)
    validate(grasp_optimizer, optimization_config, valid_data[:1], log=log)
    history = []
    for k in range(start_n_fit, n_fits):
        i_epoch, e_epoch = k * eval_after_epochs, (k + 1) * eval_after_epochs
        history += fit(grasp_model, data_generator, epochs=e_epoch, initial_epoch=i_epoch, log=log)
        results = validate(grasp_optimizer, optimization_config, valid_data, log=log)
        with open(f'{model_log_dir}/valid/results-{e_epoch}.pkl', 'wb') as f:
            pickle.dump(results, f)
        log_results(e_epoch, results, callback, print_fn=log)
        new_mean_error = np.mean(np.stack([r['errors_r'][-1] for r in results], axis=0), axis=0)
        if combined_error(new_mean_error) < combined_error(best_mean_error):
            grasp_model.store(f'{model_log_dir}/best')
            best_mean_error = [float(e) for e in new_mean_error]
            log(f'New best mean error: {best_mean_error[0] * 1000}, {best_mean_error[1] / np.pi * 180}')
        with open(training_progress_file, 'w') as f:
            json.dump({'epoch': e_epoch, 'best_mean_error': [float(e) for e in best_mean_error]}, f)
        grasp_model.store(model_checkpoint_name)
    return history


def select_loss(name):
    """train_language.py:40-63 -> (loss, softmax_before_loss)."""
    if name == 'cross_entropy':
        return categorical_crossentropy_from_logits, False
    if name == 'kl_divergence':
        return kl_divergence, True
    raise ValueError(f'Loss {name} not supported.')


def _size(text):
    h, _, w = str(text).partition('x')
    return int(h), int(w or h)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--model-path', default='/tmp/language_run', help='grasp_training.model_path')
    ap.add_argument('--backbone-path', default='/tmp/mvnerf_run', help='grasp_training.backbone_path (reads <path>/model_final_*)')
    ap.add_argument('--init-backbone', action='store_true', help='first store a random glorot backbone there (synthetic runs)')
    ap.add_argument('--epochs', type=int, default=4, help='grasp_training.n_epochs (reference 400)')
    ap.add_argument('--eval-after', type=int, default=2, help='grasp_training.eval_after_epochs (reference 4)')
    ap.add_argument('--batch-size', type=int, default=8)
    ap.add_argument('--learning-rate', type=float, default=1e-4)
    ap.add_argument('--loss', default='kl_divergence', choices=['kl_divergence', 'cross_entropy'])
    ap.add_argument('--n-views', type=int, default=1, help='nerf_model.n_views')
    ap.add_argument('--pose-augmentation-factor', type=int, default=32)
    ap.add_argument('--n-future-poses', type=int, default=6)
    ap.add_argument('--rotation-representation', default='6d', choices=['6d', 'quaternion'])
    ap.add_argument('--n-initial-guesses', type=int, default=4096)
    ap.add_argument('--n-images', type=int, default=3)
    ap.add_argument('--n-optimization-steps', type=int, default=16)
    ap.add_argument('--init-lr-t', type=float, default=0.05)
    ap.add_argument('--init-lr-r', type=float, default=0.05)
    ap.add_argument('--decay-t', type=float, default=0.9)
    ap.add_argument('--decay-r', type=float, default=0.09)
    ap.add_argument('--valid-samples', type=int, nargs='+', default=[0, 4, 7], help='validation.valid_sample_indices')
    ap.add_argument('--graph', action='store_true', help='compile(graph=True) on the grasp model and the pose optimiser')
    ap.add_argument('--fused-validation', action='store_true',
                    help='compile(fused=True) on the validation pose optimiser: its step as one C call (mvnerf_grasp_opt_step)')
    ap.add_argument('--fused-tail', action='store_true',
                    help="compile(fused_tail=True): the read-out's per-pose layers as fused HIP passes (csrc/grasp_tail_train.hip)")
    ap.add_argument('--fused-step', action='store_true',
                    help='compile(fused_step=True): the training step up to the optimiser as one C call (csrc/language_api.hip)')
    ap.add_argument('--fused-optimizer', action='store_true',
                    help='compile(fused_optimizer=True): the whole training step, clip + Keras Adam included, as one C call '
                         '(csrc/language_opt.hip); implies --fused-step')
    ap.add_argument('--size', default='32', help='image size: H or HxW (reference 480x640)')
    ap.add_argument('--n-scenes', type=int, default=16)
    ap.add_argument('--n-perspectives', type=int, default=5)
    ap.add_argument('--encoder', default='none', choices=['none', 'v4'],
                    help="where the feature maps come from: 'none' the synthetic bump map; 'v4' encoders.LanguageFeatureProducer "
                         '(CombineCLIPVisualV4 on CLIP stand-ins) on each view and the tokens of its instruction')
    ap.add_argument('--fused-conv', action='store_true',
                    help="with --encoder v4: the fusion's 3x3 convolutions as HIP launches (LanguageFeatureProducer(fused_conv='auto'); "
                         'csrc/conv3x3.hip)')
    ap.add_argument('--fused-visual', action='store_true',
                    help="with --encoder v4: the 3x3 convolutions and batch-statistics normalisations of VisualFeatures as HIP passes "
                         "(LanguageFeatureProducer(fused_visual='auto'); csrc/conv3x3.hip, csrc/batchnorm.hip)")
    ap.add_argument('--fused-vit', action='store_true',
                    help="with --encoder v4: the transformer blocks of the ViT of VisualFeatures as HIP passes "
                         "(LanguageFeatureProducer(fused_vit='auto'); csrc/token_linear.hip, csrc/attention.hip)")
    ap.add_argument('--host-batches', action='store_true', help='assemble batches in NumPy on the host (default: on the GPU)')
    args = ap.parse_args(argv)
    if args.fused_conv and args.encoder != 'v4':
        ap.error('--fused-conv needs --encoder v4')
    if args.fused_visual and args.encoder != 'v4':
        ap.error('--fused-visual needs --encoder v4')
    if args.fused_vit and args.encoder != 'v4':
        ap.error('--fused-vit needs --encoder v4')
    height, width = _size(args.size)
    bounds = DEFAULT_WORKSPACE_BOUNDS
    dev = 'cuda:0'
    train = SyntheticLanguageDataset(args.n_scenes, args.n_perspectives, height, width, bounds, seed=0)
    valid = SyntheticLanguageDataset(max(args.valid_samples) + 1, args.n_perspectives, height, width, bounds, seed=1)
    with_tokens = args.encoder == 'v4'
    if with_tokens:
        from .encoders import LanguageFeatureProducer
        # a fusion file written by the renderer (use_dense=False: `Slice` has no variable) decides the producer's own setting
        fusion_file = os.path.join(args.backbone_path, 'model_final_combine_clip_visual.pt')
        combine_kw = None
        if os.path.exists(fusion_file) and not any('.tile.dense.' in key for key in torch.load(fusion_file, weights_only=True)):
            combine_kw = dict(use_dense=False)
        producer = LanguageFeatureProducer((height, width), combine_kw=combine_kw, fused_conv='auto' if args.fused_conv else False,
                                           fused_visual='auto' if args.fused_visual else False,
                                           fused_vit='auto' if args.fused_vit else False).to(dev)
        train, valid = (EncodedLanguageDataset(d, producer, None if args.host_batches else dev) for d in (train, valid))
    generator = LanguageDataGenerator(train, bounds, n_views=args.n_views, batch_size=args.batch_size,
                                      pose_augmentation_factor=args.pose_augmentation_factor, n_future_poses=args.n_future_poses,
                                      rotation_representation=args.rotation_representation, device=None if args.host_batches else dev,
                                      with_tokens=with_tokens)
    loss, softmax_before_loss = select_loss(args.loss)
    model = LanguageNeRF(np.zeros(NET_PARAMS, dtype=np.float32), n_points_train=args.pose_augmentation_factor * args.n_future_poses,
                         n_views=args.n_views, batch_size=args.batch_size, rotation_representation=args.rotation_representation,
                         softmax_before_loss=softmax_before_loss, device=dev)
    fused_step = args.fused_step or args.fused_optimizer
    model.compile(loss=loss, learning_rate=args.learning_rate, graph=args.graph, fused_tail=args.fused_tail, fused_step=fused_step,
                  fused_optimizer=args.fused_optimizer)
    backbone = os.path.join(args.backbone_path, 'model_final')
    if args.init_backbone:
        os.makedirs(args.backbone_path, exist_ok=True)
        store_trunk(backbone, glorot_net(np.random.default_rng(0)))
    # a renderer trained with `train_nerf --encoder v4` also left its two encoder files (MVVNeRFRenderer.store(encoders=True)): they go
    # into the producer before it computes its first feature map (model_v4.py:132-152); without them the producer keeps its initial weights
    encoder_files = with_tokens and all(os.path.exists(f'{backbone}_{name}.pt') for name in ('visual_features', 'combine_clip_visual'))
    if model.load_backbone(backbone, producer=producer if encoder_files else None):
        print(f'Backbone loaded from {backbone}' + (' (with visual_features and combine_clip_visual).' if encoder_files else '.'))
    else:
        raise FileNotFoundError(f'Model not found at {backbone}.')
    os.makedirs(f'{args.model_path}/valid', exist_ok=True)
    checkpoint = f'{args.model_path}/model_final'
    print(f'Model loaded from {checkpoint}.' if model.load(checkpoint) else 'New model initialized.')
    optimizer = DNGFOptimizer(model, workspace_bounds=bounds, n_initial_guesses=args.n_initial_guesses, n_images=args.n_images,
                              clip_translation=True, rotation_representation=args.rotation_representation)
    optimizer.compile(graph=args.graph, fused=args.fused_validation)
    valid_data = [get_inputs(valid, i, args.n_images, device=dev, with_tokens=with_tokens) for i in args.valid_samples]
    optimization_config = dict(n_optimization_steps=args.n_optimization_steps, init_lr_t=args.init_lr_t, init_lr_r=args.init_lr_r,
                               decay_t=args.decay_t, decay_r=args.decay_r)
    start = time.time()
    train_grasp_model(model, generator, args.epochs, args.eval_after, args.model_path, checkpoint, optimizer, optimization_config, None,
                      valid_data, fused_tail=args.fused_tail, fused_step=fused_step, fused_optimizer=args.fused_optimizer)
    print(f'done in {time.time() - start:.1f} s')


if __name__ == '__main__':
    main()
