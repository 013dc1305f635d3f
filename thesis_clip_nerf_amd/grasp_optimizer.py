"""Grasp-pose optimisation through a trained `LanguageNeRF` (reference: src/lib/lmvnerf/grasp_optimizer.py:28-184, driven by
src/utils/optimization.py:40-152).

`DNGFOptimizer` holds P candidate grasp poses (translations (1, P, 3), rotations (1, P, 4) quaternion or (1, P, 6) 6d) and moves them by
gradient ascent on the frozen grasp model's predicted success: loss = -sum over scenes of success, clip-by-value 1, Keras Adam with an
exponentially decaying rate (one optimiser per variable), then post_process (clip t to the workspace, renormalise the rotation).

One step is an explicit pipeline, not autograd over the whole model:
  1. mvnerf_pose_query_points      poses -> query points / directions of every (pose, gripper offset), once per scene
  2. query_stash + stash_fused_acts the frozen trunk on those points, pre-activations kept for its VJP
  3. grasp_head_fwd                 the per-point part of GraspReadout
  4. the per-pose GraspReadout blocks in torch, autograd over this small sub-graph only (weights detached: no weight gradients)
  5. grasp_head_vjp                 -> cotangents of the trunk activations
  6. query_vjp                      -> cotangents of the query points / directions
  7. mvnerf_pose_query_vjp          -> d(-success)/d(t, rot), fixed-order per-pose sums
  8. mvnerf_pose_adam_step          clip, Adam with the decayed rate computed on the device, post_process
Nothing per step comes from the host, so `compile(graph=True)` captures one step and replays it for both phases (the phase is a
device-side flag pair).  `compile(fused=True)` runs the same eight stages behind the C ABI instead - stage 4 as the HIP kernels of
csrc/grasp_tail.hip, stage 5 writing g_acts only, the whole step one call of mvnerf_grasp_opt_step on a workspace allocated in `bind()` -
so that no torch module, autograd graph or per-step allocation is left in it.  TF / scipy semantics restated here are
parity-unpinned, like the other third-party definitions.
"""
from __future__ import annotations

import time
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .lmvnerf import COMPUTE_DTYPES, N_FUSED, TrunkState, rotation_from_6d, rotation_from_quaternion, t_m_to_h_matrix

DEFAULT_WORKSPACE_BOUNDS = ((0.35, 0.85), (-0.25, 0.25), (0.0, 0.2))      # configs/generator_grasp/default.yaml


@dataclass(frozen=True)
class KerasAdam:
    """tf.keras.optimizers.Adam(learning_rate=ExponentialDecay(init_lr, decay_steps=1, decay_rate, staircase=False)) as
    optimization.py:47-61 builds it (TF 2.11 optimizer: beta_1 0.9, beta_2 0.999, epsilon 1e-7)."""
    init_lr: float = 0.09
    decay_rate: float = 1.0
    beta_1: float = 0.9
    beta_2: float = 0.999
    epsilon: float = 1e-7


def euler_xyz_to_matrix(rpy):
    """scipy Rotation.from_euler('xyz', rpy).as_matrix() (extrinsic x, then y, then z: Rz Ry Rx), float64, rpy (..., 3)."""
    a, b, c = (np.asarray(rpy, dtype=np.float64)[..., i] for i in range(3))
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    m = np.stack([cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa,
                  sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa,
                  -sb, cb * sa, cb * ca], -1)
    return m.reshape(m.shape[:-1] + (3, 3))


def euler_xyz_to_quat(rpy):
    """scipy Rotation.from_euler('xyz', rpy).as_quat() (x, y, z, w): the composition q_z q_y q_x of the elementary half-angle quaternions,
    with the sign that composition gives."""
    h = np.asarray(rpy, dtype=np.float64) * 0.5
    ca, sa, cb, sb, cc, sc = np.cos(h[..., 0]), np.sin(h[..., 0]), np.cos(h[..., 1]), np.sin(h[..., 1]), np.cos(h[..., 2]), np.sin(h[..., 2])
    return np.stack([cc * cb * sa - sc * ca * sb, cc * ca * sb + sc * cb * sa, sc * ca * cb - cc * sa * sb, cc * ca * cb + sc * sa * sb], -1)


class DNGFOptimizer:
    """grasp_optimizer.py:28-184 on the HIP trunk.  `nerf_grasper` is a `LanguageNeRF`; its `n_views` views form one scene, the
    `n_images` input images are regrouped into B = n_images / n_views scenes."""

    def __init__(self, nerf_grasper, workspace_bounds=DEFAULT_WORKSPACE_BOUNDS, n_initial_guesses=32, n_images=3, fixed_orientation=None,
                 clip_translation=False, rotation_representation='quaternion', compute_dtype='f32'):
        if rotation_representation not in ('quaternion', '6d'):
            raise ValueError('Unknown rotation representation: ' + rotation_representation)
        if compute_dtype not in COMPUTE_DTYPES:
            raise ValueError(f"compute_dtype must be 'f32' or 'bf16', got {compute_dtype!r}")
        self.compute_dtype = compute_dtype          # 'bf16': stages 2 and 6 on the bf16 MFMA (query_stash_bf16, query_vjp_bf16)
        self.workspace_bounds = np.array(workspace_bounds, dtype=np.float64)
        if self.workspace_bounds.shape != (3, 2):
            raise ValueError(f'workspace_bounds: shape {self.workspace_bounds.shape}, expected (3, 2)')
        self.nerf_grasper = nerf_grasper
        self.n_initial_guesses = int(n_initial_guesses)
        self.n_images = int(n_images)
        n_views = int(nerf_grasper.n_views)
        if self.n_images <= 0 or self.n_images % n_views != 0:
            raise ValueError(f'n_images = {n_images} is not a multiple of the grasp model\'s n_views = {n_views}')
        self.batch_size = self.n_images // n_views
        self.fixed_orientation = fixed_orientation          # accepted, as the reference does; not used by its optimisation either
        self.clip_translation = bool(clip_translation)
        self.rotation_representation = rotation_representation
        self.device_ = nerf_grasper.device_
        p, rd = self.n_initial_guesses, (4 if rotation_representation == 'quaternion' else 6)
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=self.device_)
        self.translations, self.rotations = z(1, p, 3), z(1, p, rd)
        self.pose_variables = [self.translations, self.rotations]
        # Adam state of both variables, step counters (2, P) and the phase flags (2,): device buffers at fixed addresses (graph replay)
        self._m_t, self._v_t, self._m_r, self._v_r = z(p, 3), z(p, 3), z(p, rd), z(p, rd)
        self._counters, self._flags = z(2, p, dt=torch.int32), z(2, dt=torch.int32)
        self._flags_host = (0, 0)
        self._g_t, self._g_r = z(p, 3), z(p, rd)
        self.optimizer = None
        self._adam_cfg = None
        self._graph_mode = False
        self._fused = False
        self._bound = None
        self._graph, self._g_out, self._g_calls, self._g_cfg = None, None, 0, None

    # -- reference API --
    def compile(self, optimizer=None, graph=None, fused=None):
        """optimizer: [translations, rotations] as two `KerasAdam` (the reference passes two keras Adams, optimization.py:61-62), or one
        for both.  A new optimiser starts fresh: moments and step counters are zeroed.  graph=True: `optimize_pose` runs two steps
        eagerly, captures the third as a HIP graph and replays it from then on (None keeps the current mode).  fused=True: the step,
        `success_and_gradients` and `compute_current_grasp_success` are single calls of the C entry points mvnerf_grasp_opt_step /
        _success_and_gradients / _success (None keeps the current mode; changing it drops a captured graph)."""
        if fused is not None and not isinstance(fused, bool):
            raise ValueError(f'fused: expected None, True or False, got {fused!r}')
        if optimizer is None:
            optimizer = [KerasAdam(), KerasAdam()]
        if isinstance(optimizer, KerasAdam):
            optimizer = [optimizer, optimizer]
        opt_t, opt_r = optimizer
        if (opt_t.beta_1, opt_t.beta_2, opt_t.epsilon) != (opt_r.beta_1, opt_r.beta_2, opt_r.epsilon):
            raise ValueError('the two optimisers must share beta_1, beta_2 and epsilon (one fused update)')
        self.optimizer = [opt_t, opt_r]
        self._adam_cfg = ops.pose_adam_config(lr0=(opt_t.init_lr, opt_r.init_lr), decay=(opt_t.decay_rate, opt_r.decay_rate),
                                              beta1=opt_t.beta_1, beta2=opt_t.beta_2, eps=opt_t.epsilon, clip=1.0,
                                              clip_translation=self.clip_translation, bounds=self.workspace_bounds)
        for buf in (self._m_t, self._v_t, self._m_r, self._v_r, self._counters):
            buf.zero_()
        if graph is not None:
            self._graph_mode = bool(graph)
        if fused is not None and fused != self._fused:
            self._fused = fused
            self._graph, self._g_out, self._g_calls = None, None, 0
        key = self._cfg_key()
        if self._g_cfg != key:                 # the captured launch holds the configuration as kernel arguments
            self._graph, self._g_out, self._g_calls = None, None, 0

    def _cfg_key(self):
        c = self._adam_cfg
        return (tuple(c.lr0), tuple(c.decay), c.beta1, c.beta2, c.eps, c.clip, c.clip_translation, tuple(c.lo), tuple(c.hi))

    def set_initial_guesses(self, initial_guesses):
        if len(initial_guesses) != 2:
            raise ValueError('initial_guesses: expected [translations, rotations]')
        rd = self.rotations.shape[-1]
        t, r = (torch.as_tensor(np.asarray(g) if not isinstance(g, torch.Tensor) else g, dtype=torch.float32) for g in initial_guesses)
        if tuple(t.shape) != (1, self.n_initial_guesses, 3):
            raise ValueError(f'translations: shape {tuple(t.shape)}, expected {(1, self.n_initial_guesses, 3)}')
        if tuple(r.shape) != (1, self.n_initial_guesses, rd):
            raise ValueError(f'rotations: shape {tuple(r.shape)}, expected {(1, self.n_initial_guesses, rd)}')
        self.translations.copy_(t)
        self.rotations.copy_(r)

    def generate_initial_guesses(self, workspace_bounds=None, n_initial_guesses=None, batch_size=1, rng=None):
        """grasp_optimizer.py:72-94 with Affine.random (manipulation_tasks/transform.py:32-55): t ~ U(bounds), rpy ~ U[0, 2 pi)^3,
        R = scipy from_euler('xyz', rpy); quaternion = its as_quat (x, y, z, w), 6d = [R[:, 0], R[:, 1]].  float64 arrays
        (batch_size, P, 3), (batch_size, P, 4|6).  rng: a numpy Generator / RandomState (default: numpy's global state, as the
        reference); per pose the six draws come in the reference's order (t, then rpy)."""
        bounds = self.workspace_bounds if workspace_bounds is None else np.asarray(workspace_bounds, dtype=np.float64)
        n = self.n_initial_guesses if n_initial_guesses is None else int(n_initial_guesses)
        rng = np.random if rng is None else rng
        lo = np.concatenate([bounds[:, 0], np.zeros(3)])
        hi = np.concatenate([bounds[:, 1], np.full(3, 2 * np.pi)])
        ts, rs = [], []
        for _ in range(batch_size):
            draw = rng.uniform(lo, hi, size=(n, 6))
            ts.append(draw[:, :3])
            if self.rotation_representation == 'quaternion':
                rs.append(euler_xyz_to_quat(draw[:, 3:]))
            else:
                m = euler_xyz_to_matrix(draw[:, 3:])
                rs.append(np.concatenate([m[:, :, 0], m[:, :, 1]], -1))
        return [np.array(ts), np.array(rs)]

    def compute_matrices(self):
        rot = rotation_from_quaternion(self.rotations) if self.rotation_representation == 'quaternion' else rotation_from_6d(self.rotations)
        return t_m_to_h_matrix(self.translations, rot)

    def get_results(self):
        """The current poses as (P, 4, 4) float32 matrices (the reference returns a list of Affine made from them)."""
        return self.compute_matrices()[0].cpu().numpy()

    def post_process(self):
        """grasp_optimizer.py:126-139 (the optimisation step runs it inside mvnerf_pose_adam_step)."""
        if self.clip_translation:
            b = torch.as_tensor(self.workspace_bounds, dtype=torch.float32, device=self.device_)
            self.translations.copy_(torch.minimum(torch.maximum(self.translations, b[:, 0]), b[:, 1]))
        if self.rotation_representation == 'quaternion':
            self.rotations.copy_(self.rotations / self.rotations.norm(dim=-1, keepdim=True))
        else:
            r = self.rotations
            self.rotations.copy_(torch.cat([r[..., :3] / r[..., :3].norm(dim=-1, keepdim=True),
                                            r[..., 3:] / r[..., 3:].norm(dim=-1, keepdim=True)], -1))

    def regroup(self, input_data, features):
        """(images (1, n_images, H, W, 3), intrinsics, extrinsics_inv (1, n_images, 4, 4)), features (1, n_images, H, W, 256) -> the same as
        (B, n_views, ...) views (grasp_optimizer.py:141-166: 'b nv ... -> nv b ...' for n_views == 1, unchanged for B == 1)."""
        dev, nv, b = self.device_, self.nerf_grasper.n_views, self.batch_size
        out = []
        for name, x in zip(('images', 'intrinsics', 'extrinsics_inv', 'features'), (*input_data[:3], features)):
            x = torch.as_tensor(x, dtype=torch.float32).to(dev)
            if x.dim() < 2 or x.shape[0] * x.shape[1] != self.n_images:
                raise ValueError(f'{name}: shape {tuple(x.shape)}, expected (1, n_images = {self.n_images}, ...)')
            out.append(x.reshape((b, nv) + tuple(x.shape[2:])))
        return out

    def device_inputs(self, input_data, features):
        """The inputs as float32 tensors on the model's device: device tensors are returned as they are (nothing is copied), host arrays
        are copied once."""
        f = lambda x: x if isinstance(x, torch.Tensor) and x.device == self.device_ and x.dtype == torch.float32 else (
            torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x, dtype=torch.float32).to(self.device_).contiguous())
        return [f(x) for x in input_data[:3]], f(features)

    def call(self, inputs, training=False, mask=None):
        """grasp_optimizer.py:96-102 through LanguageNeRF.infer (the matrix path): inputs = [[images, intrinsics, extrinsics_inv], features]
        already grouped into B scenes -> success (B, P)."""
        (images, k, einv), feats = inputs[0][:3], inputs[1]
        matrices = self.compute_matrices().expand(self.batch_size, -1, -1, -1)
        return self.nerf_grasper.infer((None, None, None, None, images, k, einv), matrices, self.n_initial_guesses, feats)

    # -- the explicit step --
    def bind(self, input_data, features):
        """Build the trunk state for these inputs (once per compute_results) and the step's fixed buffers.  The inputs are used in place
        (views, no copies).  Binding the same tensors again only refreshes the packed weights, so a captured step stays valid."""
        images, k, einv, feats = self.regroup(input_data, features)
        g = self.nerf_grasper
        key = tuple((t.data_ptr(), tuple(t.shape)) for t in (images, k, einv, feats))
        ro = g.grasp_readout
        w4 = torch.stack([lin.weight.detach() for lin in ro.activation_downscale]).contiguous()
        b4 = torch.stack([lin.bias.detach() for lin in ro.activation_downscale]).contiguous()
        wc, bc = ro.combined_activation_downscale.weight.detach().contiguous(), ro.combined_activation_downscale.bias.detach().contiguous()
        bf16 = self.compute_dtype == 'bf16'
        state = TrunkState(images, feats, k, einv, g.trunk_net, self.compute_dtype)
        head = ops.grasp_head_pack(w4, wc)
        if self._bound is not None and self._bound['key'] == key:
            bd = self._bound
            for old, new in ((bd['state'].packed, state.packed), (bd['state'].packed_split, state.packed_split),
                             (bd['state'].bwd_streams, state.bwd_streams), (bd['head'], head), (bd['b4'], b4), (bd['bc'], bc)):
                old.copy_(new)
            if bf16:
                bd['state'].packed16.copy_(state.packed16)
                bd['state'].bwd16.copy_(state.bwd16)
            if 'fused' in bd:
                self._pack_tail(out=bd['fused']['tail'])
            return bd
        b, v = self.batch_size, g.n_views
        n5 = g.n_transforms_to_check
        n = self.n_initial_guesses * n5
        ld = n + ((-n) % 32 if v > 1 else 0)          # TrunkField's rule: the multi-view kernels want whole 32-point tiles per scene
        dev = self.device_
        self._bound = dict(key=key, state=state, head=head, b4=b4, bc=bc, n=n, ld=ld, n5=n5,
                           points=torch.zeros((b, ld, 3), dtype=torch.float32, device=dev),
                           dirs=torch.zeros((b, ld, 3), dtype=torch.float32, device=dev),
                           stash=torch.empty(ops.relu_bits_bytes(b, v, ld) if bf16 else ops.stash_bytes(b, v, ld, 1), dtype=torch.uint8, device=dev),
                           g_pad=torch.zeros((N_FUSED, b, ld, 128), dtype=torch.float32, device=dev) if ld > n else None,
                           tail={name: {k_: p.detach() for k_, p in getattr(ro, name).named_parameters()}
                                 for name in ('block_0', 'block_1', 'output_layer')})
        self._graph, self._g_out, self._g_calls = None, None, 0
        if self._fused:
            self._fused_state()
        return self._bound

    def _pack_tail(self, out=None):
        ro = self.nerf_grasper.grasp_readout
        d = lambda lin: (lin.weight.detach().contiguous(), None if lin.bias is None else lin.bias.detach().contiguous())
        (w0, b0), (w1, b1), (ws, _) = d(ro.block_0.layer_0), d(ro.block_0.layer_1), d(ro.block_0.shortcut)
        (w0b, b0b), (w1b, b1b) = d(ro.block_1.layer_0), d(ro.block_1.layer_1)
        return ops.grasp_tail_pack((w0, b0, w1, b1, ws), (w0b, b0b, w1b, b1b), d(ro.output_layer), out=out)

    def _fused_state(self):
        """The fused step's buffers for the bound inputs: the packed tail, the workspace, success (B, P) and the filled mvnerf_grasp_call.
        Built once per binding (in `bind()` when fused is on, or at the first fused call after it was switched on)."""
        bd, g = self._bound, self.nerf_grasper
        if 'fused' not in bd:
            st, b, p = bd['state'], self.batch_size, self.n_initial_guesses
            dev = self.device_
            tail = self._pack_tail()
            ws = torch.empty(ops.grasp_workspace_bytes(b, g.n_views, p, bd['n5'], bf16=self.compute_dtype == 'bf16'), dtype=torch.uint8, device=dev)
            success = torch.zeros((b, p), dtype=torch.float32, device=dev)
            offsets = g.transforms_to_check.contiguous()
            call = ops.grasp_call(*st.geo, st.packed, st.packed_split, st.bwd_streams, bd['head'], bd['b4'], bd['bc'], tail, offsets,
                                  self.translations, self.rotations, success, self._g_t, self._g_r, ws)
            nets16 = (st.packed16, st.bwd16) if self.compute_dtype == 'bf16' else None       # -> the _bf16 entry points
            bd['fused'] = dict(tail=tail, ws=ws, success=success, offsets=offsets, call=call, nets16=nets16)
        return bd['fused']

    def _readout_tail(self, x):
        """GraspReadout after the fused head (delta_ngf/layers.py:38-42) with the bound, detached weights: x (B, P, n5 * 64) -> (B, P)."""
        ro, tail = self.nerf_grasper.grasp_readout, self._bound['tail']
        call = torch.func.functional_call
        x = call(ro.block_1, tail['block_1'], (call(ro.block_0, tail['block_0'], (x,)),))
        return call(ro.output_layer, tail['output_layer'], (torch.relu(x),))[..., 0]

    def _forward(self):
        """Steps 1-3: -> (c, y) of the fused head; the stash and query tensors stay in the bound buffers."""
        bd, g = self._bound, self.nerf_grasper
        st, n, ld, b = bd['state'], bd['n'], bd['ld'], self.batch_size
        points, dirs = ops.pose_query_points(self.translations, self.rotations, g.transforms_to_check, b, ld, out=(bd['points'], bd['dirs']))
        if ld > n:
            points[:, n:] = points[:, n - 1:n]
            dirs[:, n:] = dirs[:, n - 1:n]
        if self.compute_dtype == 'bf16':
            acts, _ = ops.query_stash_bf16(points, dirs, *st.geo, st.packed, st.packed16, relu_bits=bd['stash'])
        else:
            ops.query_stash(points, dirs, *st.geo, st.packed, stash=bd['stash'], packed_split=st.packed_split)
            acts = ops.stash_fused_acts(bd['stash'], b, g.n_views, ld)
        if ld > n:
            acts = acts[:, :, :n].contiguous()
        return ops.grasp_head_fwd(acts.reshape(N_FUSED, -1, 128), bd['head'], bd['b4'], bd['bc'])

    def success_and_gradients(self):
        """Steps 1-7 on the bound inputs: -> success (B, P), and d(-sum success)/d(t, rot) in the step's gradient buffers (P, 3), (P, 4|6)."""
        if self._fused:
            fs = self._fused_state()
            ops.grasp_success_and_gradients(fs['call'], self.translations, nets16=fs['nets16'])
            return fs['success'].clone(), self._g_t, self._g_r
        bd, g = self._bound, self.nerf_grasper
        st, n, ld, b, n5 = bd['state'], bd['n'], bd['ld'], self.batch_size, bd['n5']
        c, y = self._forward()
        with torch.enable_grad():
            x = y.view(b, self.n_initial_guesses, n5 * 64).detach().requires_grad_(True)
            success = self._readout_tail(x)
            (g_x,) = torch.autograd.grad(success.sum(), x)
        _, _, _, g_acts = ops.grasp_head_vjp(g_x.reshape(-1, 64).contiguous(), c, y, bd['head'])
        g_acts = g_acts.view(N_FUSED, b, n, 128)
        if ld > n:
            bd['g_pad'][:, :, :n] = g_acts
            g_acts = bd['g_pad']
        if self.compute_dtype == 'bf16':
            d_points, d_dirs = ops.query_vjp_bf16(bd['points'], bd['dirs'], *st.geo, st.bwd_streams, st.bwd16, bd['stash'], g_acts)
        else:
            d_points, d_dirs = ops.query_vjp(bd['points'], bd['dirs'], *st.geo, st.bwd_streams, bd['stash'], g_acts)
        ops.pose_query_vjp(self.rotations, g.transforms_to_check, d_points, d_dirs, scale=-1.0, out=(self._g_t, self._g_r))
        return success.detach(), self._g_t, self._g_r

    def _step(self):
        if self._fused:
            fs = self._fused_state()
            ops.grasp_opt_step(fs['call'], self._adam_cfg, self._flags, self._counters, self._m_t, self._v_t, self._m_r, self._v_r,
                               self.translations, nets16=fs['nets16'])
            return fs['success']
        success, g_t, g_r = self.success_and_gradients()
        ops.pose_adam_step(self._adam_cfg, self._flags, self._counters, g_t, g_r, self._m_t, self._v_t, self._m_r, self._v_r,
                           self.translations, self.rotations)
        return success

    def _step_graphed(self):
        if self._g_calls < 2:                    # the first two steps load every kernel and size the allocator pools
            self._g_calls += 1
            dev = self.device_
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                out = self._step()
            torch.cuda.current_stream(dev).wait_stream(side)
            return out
        if self._graph is None:
            torch.cuda.synchronize(self.device_)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self._step()
            self._graph, self._g_out, self._g_cfg = graph, out, self._cfg_key()
        self._graph.replay()
        return self._g_out.clone()

    def set_train_config(self, train_config):
        """The phase: which variables (translations, rotations) the next steps train; a device-side fill of the flag pair."""
        flags = tuple(int(bool(f)) for f in train_config)
        if len(flags) != 2:
            raise ValueError('train_config: expected two flags (translations, rotations)')
        for i in range(2):
            if flags[i] != self._flags_host[i]:
                self._flags[i].fill_(flags[i])
        self._flags_host = flags

    def optimize_pose(self, inputs, features, train_config):
        """grasp_optimizer.py:158-184: one step on (input_data, features) -> {'loss': success (P, 1)} of the poses before the step."""
        if self.optimizer is None:
            self.compile()
        if self._bound is None or self._bound['key'] != tuple((t.data_ptr(), tuple(t.shape)) for t in self.regroup(inputs, features)):
            self.bind(inputs, features)
        self.set_train_config(train_config)
        with torch.no_grad():
            success = self._step_graphed() if self._graph_mode else self._step()
        return {'loss': success.sum(0)[:, None]}

    def compute_current_grasp_success(self, inputs, features):
        """grasp_optimizer.py:141-156 -> (P, 1): success summed over the B scenes."""
        if self._bound is None or self._bound['key'] != tuple((t.data_ptr(), tuple(t.shape)) for t in self.regroup(inputs, features)):
            self.bind(inputs, features)
        b, n5 = self.batch_size, self._bound['n5']
        if self._fused:
            fs = self._fused_state()
            ops.grasp_success(fs['call'], self.translations, nets16=fs['nets16'])
            return fs['success'].sum(0)[:, None]
        with torch.no_grad():
            _, y = self._forward()
            success = self._readout_tail(y.reshape(b, self.n_initial_guesses, n5 * 64))
        return success.sum(0)[:, None]


# ---- the loop (src/utils/optimization.py) -------------------------------------------------------------------------------------------------
def optimize_pose(pose_optimizer, input_data, batched_features, train_config, n_optimization_steps=16, return_trajectory=False):
    """optimization.py:136-152 -> (optimized_grasps (P, 4, 4), losses (P,), duration [s], step_poses).  duration ends in a device
    synchronise (the losses are read back)."""
    start = time.time()
    step_poses = []
    for _ in range(n_optimization_steps):
        pose_optimizer.optimize_pose(input_data, batched_features, train_config=train_config)
        step_poses.append(pose_optimizer.get_results() if return_trajectory else [])
    optimized_grasps = pose_optimizer.get_results()
    step_poses.append(optimized_grasps)
    losses = pose_optimizer.compute_current_grasp_success(input_data, batched_features).cpu().numpy().squeeze(-1)
    duration = time.time() - start
    return optimized_grasps, losses, duration, step_poses


def compute_results(pose_optimizer, input_data, features, return_trajectory, init_poses=None, reset_optimizer=True, n_optimization_steps=1,
                    init_lr_t=0.09, decay_t=None, init_lr_r=None, decay_r=None, sync=False, rng=None):
    """optimization.py:40-105 -> (losses_t, losses_r, grasps_t, grasps_r, duration, all_poses).  decay None means no decay (rate 1.0; the
    reference would fail on it).  rng: passed to generate_initial_guesses when init_poses is None."""
    input_data, features = pose_optimizer.device_inputs(input_data, features)
    if reset_optimizer:
        init_lr_r = init_lr_t if init_lr_r is None else init_lr_r
        decay_r = decay_t if decay_r is None else decay_r
        rate = lambda d: 1.0 if d is None else float(d)
        pose_optimizer.compile(optimizer=[KerasAdam(init_lr_t, rate(decay_t)), KerasAdam(init_lr_r, rate(decay_r))])
    if init_poses is None:
        init_poses = [g[:1] for g in pose_optimizer.generate_initial_guesses(rng=rng)]
    pose_optimizer.set_initial_guesses(init_poses)
    pose_optimizer.bind(input_data, features)

    duration = 0.0
    steps_list = n_optimization_steps if isinstance(n_optimization_steps, list) else [n_optimization_steps]
    all_poses = []
    if return_trajectory:
        all_poses.append(pose_optimizer.get_results())
    for o_steps in steps_list:
        if not sync:
            grasps_t, losses_t, duration_t, poses = optimize_pose(pose_optimizer, input_data, features, [True, False], o_steps, return_trajectory)
            if return_trajectory:
                all_poses.extend(poses)
            grasps_r, losses_r, duration_r, poses = optimize_pose(pose_optimizer, input_data, features, [False, True], o_steps, return_trajectory)
            if return_trajectory:
                all_poses.extend(poses)
            duration += duration_t + duration_r
        else:
            grasps_r, losses_r, duration_s, poses = optimize_pose(pose_optimizer, input_data, features, [True, True], o_steps, return_trajectory)
            losses_t, grasps_t = losses_r, grasps_r
            if return_trajectory:
                all_poses.extend(poses)
            duration += duration_s
    return losses_t, losses_r, grasps_t, grasps_r, duration, all_poses


def best_grasps(losses, poses, k=5):
    """get_step_results' selection (optimization.py:117-122): the k poses of highest final success, in ascending order of success ->
    (indices, poses[indices], losses[indices])."""
    idx = np.argsort(np.asarray(losses))[-k:]
    return idx, np.asarray(poses)[idx], np.asarray(losses)[idx]


__all__ = ['DNGFOptimizer', 'KerasAdam', 'compute_results', 'optimize_pose', 'best_grasps', 'euler_xyz_to_matrix', 'euler_xyz_to_quat',
           'DEFAULT_WORKSPACE_BOUNDS']
