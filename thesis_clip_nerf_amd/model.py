"""Host-side mirror of the reference renderer (src/lib/mvnerf/model_v0.py) on top of the HIP library.

Same names and argument meaning as the reference so that a `train_nerf.py`-style script (or a
test) reads the same:

* :class:`MVVNeRFRenderer` - ``_call`` / ``infer`` / ``call`` / ``volumetric_render`` / ``store`` /
  ``load`` (model_v0.py:16-240).  The two MLPs are held as flat Keras-order fp32 buffers
  (``kernel[in,out]``, ``bias[out]``); the image encoders (``VisualFeatures``, CLIP,
  ``CombineCLIPVisual*``) are NOT part of the hot path: their output ``combined_features``
  (B,V,H,W,256) is an input here, or comes from a user-supplied ``feature_encoder`` callable.
* :func:`render_view` (model_v0.py:243-281) - full-image driver, device resident (no per-chunk
  host round trip, source images uploaded once).
* :func:`render` - the ``render(rays, model) -> rgb, depth`` surface named in BASELINE.json.

Differences that are deliberate: image size and ray count are not baked into
signatures; the uniforms that the reference draws inside the graph with ``tf.random.uniform``
(nerf_utils.py:57,151) can be passed explicitly (``u_coarse``, ``u_fine``) and otherwise come from
``torch.rand`` on the device (optionally with a ``generator``).
"""
from __future__ import annotations

import os
import warnings

import numpy as np
import torch

from . import ops, range_policy as rp
from ._lib import NET_PARAMS, Q7_ZERO
from .synthetic import glorot_net

_SUBMODELS = ('coarse_embedding', 'coarse_readout', 'fine_embedding', 'fine_readout')
ENCODER_SUBMODELS = ('visual_features', 'combine_clip_visual')       # the renderer's other two files (mvnerf/model_v4.py:196-240)


def check_state_dict(module, state, what):
    """ValueError naming the first key of `state` that `module` lacks, misses or holds with another shape; nothing is written."""
    own = module.state_dict()
    for key in list(own) + [k for k in state if k not in own]:
        if key not in state:
            raise ValueError(f'{what}: key {key!r} is missing')
        if key not in own:
            raise ValueError(f'{what}: unexpected key {key!r}')
        if tuple(state[key].shape) != tuple(own[key].shape):
            raise ValueError(f'{what}: key {key!r} has shape {tuple(state[key].shape)}, expected {tuple(own[key].shape)}')
_EMB_PARAMS = NET_PARAMS - (128 * 4 + 4)      # trunk part of the flat buffer; the rest is the read-out


class MVVNeRFRenderer:
    """model_v0.py:16-44.  Holds the coarse and fine MLP weights and runs `_call` on the GPU."""

    def __init__(self, n_rays_train, n_rays_infer, n_views=2, n_samples=64, n_features=256,
                 embed_direction_vector=True, batch_size=1, near=0.7, far=1.5, original_image_size=(480, 640),
                 device='cuda', seed=0, feature_encoder=None, q7_mode=Q7_ZERO, compute_dtype='f32', f32_gemm='split_f16',
                 range_policy='fallback', range_check=False):
        if n_features != 256:
            raise ValueError('n_features must be 256 (the HIP kernels are built for the reference feature width)')
        if not embed_direction_vector:
            raise ValueError('embed_direction_vector=False is not built (every reference config sets True)')
        if n_samples != 64:
            raise ValueError('n_samples must be 64 (reference config nerf_model/default.yaml:3)')
        self.n_views = n_views
        self.n_samples = n_samples
        self.n_rays_train = n_rays_train
        self.n_rays_infer = n_rays_infer
        self.batch_size = batch_size
        self.infer_batch_size = 1
        self.near = near
        self.far = far
        self.original_image_size = tuple(original_image_size)
        self.device = torch.device(device)
        self.feature_encoder = feature_encoder
        self.q7_mode = q7_mode
        if compute_dtype not in ('f32', 'bf16'):
            raise ValueError("compute_dtype must be 'f32' (reference precision) or 'bf16' (bf16 MFMA inputs, fp32 accumulate)")
        self.compute_dtype = compute_dtype       # inference only; training always runs the fp32 path
        if f32_gemm not in ('split_f16', 'split_bf16', 'mfma_f32'):
            raise ValueError("f32_gemm must be 'split_f16' (two fp16 pieces per operand, three MFMAs per product block: the default), "
                             "'split_bf16' (exact three-piece bf16 cut, six MFMAs) - both fp32-grade - or 'mfma_f32'")
        self.f32_gemm = f32_gemm                 # how compute_dtype='f32' inference runs its Dense layers (same results to ~1e-6)
        # 'split_f16' is only correct for |w| < 1023, |activation| < 4.19e6 (range_policy.py).  Weights are checked once per weight
        # version by the first inference call after a change; out of range the call runs on 'split_bf16' with one RuntimeWarning
        # ('fallback'), raises FloatingPointError ('raise'), or nobody looks ('off').  Activations are opt-in (range_check=True routes
        # `_call` through the range-guarded kernel, range_report() reads the result): reading the status is a host synchronisation.
        if range_policy not in rp.POLICIES:
            raise ValueError(f'range_policy must be one of {rp.POLICIES}, got {range_policy!r}')
        self.range_policy = range_policy
        self.range_check = bool(range_check)
        self._weight_range = None       # ((max |w|, max |.|) coarse, fine) of the current weight version, once read
        self._range_status = None       # device (2,): max |cut activation| of the coarse / fine passes since range_reset()
        rng = np.random.default_rng(seed)
        self.coarse_net = torch.from_numpy(glorot_net(rng)).to(self.device)      # Keras glorot_uniform, zero bias
        self.fine_net = torch.from_numpy(glorot_net(rng)).to(self.device)
        self._packed = None
        self._packed16 = None
        self._packed_split = None
        self._packed_bwd = None
        self._workspace = None
        self._tables = None             # (2,B,V,H,W,128) texel tables [coarse | fine] of the last scene, see _call
        self._tables_key = None
        self._last_call = (None, None)  # the mvnerf_train_call of the last loss_and_grads (and the tensors it points to)

    # ---- weights -------------------------------------------------------------------------
    def set_weights(self, coarse_net=None, fine_net=None):
        """Replace the flat Keras-order buffers (247 300 fp32 each) and drop the packed images."""
        for name, val in (('coarse_net', coarse_net), ('fine_net', fine_net)):
            if val is not None:
                val = torch.as_tensor(val, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
                if val.numel() != NET_PARAMS:
                    raise ValueError(f'{name}: {val.numel()} parameters, expected {NET_PARAMS}')
                setattr(self, name, val)
        self._packed = None
        self._packed_bwd = None
        self._tables_key = None
        self._last_call = (None, None)
        self._weight_range = None

    def weights_changed(self):
        """Call after updating coarse_net / fine_net in place (e.g. an optimizer step)."""
        self._packed = None
        self._packed_bwd = None
        self._tables_key = None
        self._last_call = (None, None)
        self._weight_range = None

    def packed(self):
        if self._packed is None:
            self._packed = (ops.pack_net(self.coarse_net), ops.pack_net(self.fine_net))
            self._packed16 = None
            self._packed_split = None
        return self._packed

    def packed_split(self):
        self.packed()
        if self._packed_split is None:
            self._packed_split = (ops.pack_net_split(self.coarse_net), ops.pack_net_split(self.fine_net))
        return self._packed_split

    def packed16(self):
        self.packed()
        if self._packed16 is None:
            self._packed16 = (ops.pack_net_bf16(self.coarse_net), ops.pack_net_bf16(self.fine_net))
        return self._packed16

    # ---- range of the fp16 two-piece kernel (range_policy.py) ---------------------------------
    def weight_range(self):
        """((max |w| over the cut weights, max |.| over all variables) of the coarse net, ... of the fine net): one host read per
        weight version (ops.net_range), cached until the weights change."""
        if self._weight_range is None:
            both = torch.stack([ops.net_range(self.coarse_net), ops.net_range(self.fine_net)]).cpu().tolist()
            self._weight_range = (tuple(both[0]), tuple(both[1]))
        return self._weight_range

    def _inference_kernel(self):
        """The split kernel an inference call runs: f32_gemm, or 'split_bf16' when the weights have left split_f16's range."""
        if self.f32_gemm != 'split_f16' or self.range_policy == 'off':
            return self.f32_gemm
        first = self._weight_range is None
        max_w = rp.worst([net[0] for net in self.weight_range()])
        action = rp.decide(self.range_policy, self.f32_gemm, max_weight=max_w)
        if action == rp.RUN:
            return self.f32_gemm
        if action == rp.RAISE:
            raise FloatingPointError(rp.describe(max_w, None))
        if first:                               # one warning per weight version
            warnings.warn(rp.describe(max_w, None) + " - running on 'split_bf16'", RuntimeWarning, stacklevel=3)
        return 'split_bf16'

    def range_reset(self):
        """Zero the activation status that range-checked calls accumulate into."""
        if self._range_status is None:
            self._range_status = torch.zeros(2, dtype=torch.float32, device=self.device)
        else:
            self._range_status.zero_()
        return self._range_status

    def range_report(self):
        """Synchronises.  -> {'coarse': {'max_weight', 'max_activation'}, 'fine': {...}, 'in_range': bool}: the weights of the current
        version and the largest |activation| the range-checked calls since range_reset() cut into fp16 pieces (0.0: none ran)."""
        acts = [0.0, 0.0] if self._range_status is None else self._range_status.cpu().tolist()
        wr = self.weight_range()
        out = {name: {'max_weight': wr[k][0], 'max_activation': acts[k]} for k, name in enumerate(('coarse', 'fine'))}
        out['in_range'] = all(rp.in_range(v['max_weight'], v['max_activation']) for v in list(out.values()))
        return out

    def check_range(self, inputs, combined_features, training=True, u_coarse=None, u_fine=None, generator=None):
        """Runs the coarse -> resample -> fine chain of one step on the range-guarded training forward (ops.field_eval_stash with a
        range status) and reads the result: synchronises.  training=True compares with the backward's limit (every stashed
        pre-activation below 1023: the weight-gradient GEMM cuts relu(a) as rn16(64 a)), training=False with the forward's.
        -> {'coarse': {...}, 'fine': {...}, 'limit', 'in_range', 'message'}."""
        rays_o, rays_d, images, k4, einv = [self._dev(t) for t in inputs]
        feats = self._dev(combined_features)
        b, r, _ = rays_o.shape
        u_coarse, u_fine = self._uniforms(b, r, u_coarse, u_fine, generator)
        pc, pf = self.packed()
        sc, sf = self.packed_split()
        status = torch.zeros(2, dtype=torch.float32, device=self.device)
        geo = (images, feats, k4, einv)
        z = ops.stratified_depths(self._dev(u_coarse), self.near, self.far)
        rgbs_c, stash = ops.field_eval_stash(rays_o, rays_d, z, *geo, pc, packed_split=sc, kernel='split_f16', range_status=status[0:1])
        _, _, w = ops.composite(z, rgbs_c)
        z_all = ops.resample(z, w, self._dev(u_fine), self.q7_mode)
        del stash
        ops.field_eval_stash(rays_o, rays_d, z_all, *geo, pf, packed_split=sf, kernel='split_f16', range_status=status[1:2])
        acts = status.cpu().tolist()
        wr = self.weight_range()
        out = {name: {'max_weight': wr[k][0], 'max_activation': acts[k]} for k, name in enumerate(('coarse', 'fine'))}
        max_w, max_a = rp.worst([wr[0][0], wr[1][0]]), rp.worst(acts)
        out['limit'] = rp.limits(training)[1]
        out['in_range'] = rp.in_range(max_w, max_a, training)
        out['message'] = '' if out['in_range'] else rp.describe(max_w, max_a, training)
        return out

    # ---- forward -------------------------------------------------------------------------
    def encode(self, image):
        """model_v0.py:47-49 - image encoder hook; out of the hot-path scope."""
        if self.feature_encoder is None:
            raise NotImplementedError('no feature_encoder configured: pass combined_features explicitly '
                                      '(the conv/ViT/CLIP encoders are outside the render hot path)')
        return self.feature_encoder(image)

    def _uniforms(self, b, r, u_coarse, u_fine, generator):
        shape = (b, r, self.n_samples)
        if u_coarse is None:
            u_coarse = torch.rand(shape, dtype=torch.float32, device=self.device, generator=generator)
        if u_fine is None:
            u_fine = torch.rand(shape, dtype=torch.float32, device=self.device, generator=generator)
        return u_coarse, u_fine

    def _call(self, inputs, n_rays, batch_size, combined_features, u_coarse=None, u_fine=None, generator=None,
              scene_key=None, range_check=None, kernel=None):
        """model_v0.py:113-184.  inputs = (ray_origins (B,R,3), ray_directions (B,R,3),
        images (B,V,H,W,3) in [0,1], intrinsics (B,V,4,4), extrinsics_inv (B,V,4,4)).
        Returns (rgb, depth, fine_rgb, fine_depth).
        The feature rows of layer 0 go through per-texel tables (include/mvnerf_hip.h, "Texel table") when that is
        cheaper: always rebuilt for a call with R*S >= 2*H*W; with `scene_key` (any hashable naming the feature maps,
        e.g. one frame rendered in chunks) they are built by the first call and re-used while key and weights last.
        range_check (default: the constructor's): run the split_f16 passes range-guarded, accumulating into range_report().
        kernel: run this call on that split kernel instead of f32_gemm (render_view's fallback frame)."""
        rays_o, rays_d, images, k4, einv = [self._dev(t) for t in inputs]
        if self.compute_dtype == 'bf16' and isinstance(combined_features, torch.Tensor) and combined_features.dtype == torch.bfloat16:
            # bf16 feature maps stay bf16 (encoders.FeatureProducer(out_dtype=torch.bfloat16)): the bf16 passes read them as stored
            features = combined_features.to(self.device).contiguous()
        else:
            features = self._dev(combined_features)
        if rays_o.dim() != 3 or rays_o.shape[0] != batch_size or rays_o.shape[1] != n_rays:
            raise ValueError(f'ray_origins: shape {tuple(rays_o.shape)}, expected ({batch_size}, {n_rays}, 3)')
        u_coarse, u_fine = self._uniforms(batch_size, n_rays, u_coarse, u_fine, generator)
        pc, pf = self.packed()
        if self.compute_dtype == 'bf16':
            pc16, pf16 = self.packed16()
            return ops.render_fwd_bf16(rays_o, rays_d, images, features, k4, einv, pc, pf, pc16, pf16, self._dev(u_coarse),
                                       self._dev(u_fine), self.near, self.far, self.q7_mode)
        need = ops.render_workspace_bytes(batch_size, images.shape[1], n_rays, self.n_samples)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        v, h, w = images.shape[1:4]
        tables, ready = None, False
        if scene_key is not None or ops.texel_table_pays(n_rays, self.n_samples, h, w):
            shape = (2, batch_size, v, h, w, 128)
            if self._tables is None or tuple(self._tables.shape) != shape:
                self._tables = torch.empty(shape, dtype=torch.float32, device=self.device)
                self._tables_key = None
            tables = self._tables
            ready = scene_key is not None and self._tables_key == scene_key
            self._tables_key = scene_key
        if self.f32_gemm == 'mfma_f32':
            return ops.render_fwd(rays_o, rays_d, images, features, k4, einv, pc, pf, self._dev(u_coarse), self._dev(u_fine),
                                  self.near, self.far, self.q7_mode, workspace=self._workspace, texel_tables=tables, tables_ready=ready)
        # the split kernel is chosen for this call alone (the process-wide value is neither read nor written)
        kernel = kernel or self._inference_kernel()
        status = None
        if (self.range_check if range_check is None else range_check) and kernel == 'split_f16':
            status = self._range_status if self._range_status is not None else self.range_reset()
        return ops.render_fwd(rays_o, rays_d, images, features, k4, einv, pc, pf, self._dev(u_coarse), self._dev(u_fine),
                              self.near, self.far, self.q7_mode, workspace=self._workspace, texel_tables=tables,
                              tables_ready=ready, split=self.packed_split(), kernel=kernel, range_status=status)

    def infer(self, inputs, batched_features, **kw):
        """model_v0.py:61-63 (any ray count, not only n_rays_infer=512)."""
        return self._call(inputs, inputs[0].shape[1], inputs[0].shape[0], batched_features, **kw)

    def call(self, inputs, training=False, combined_features=None, **kw):
        """model_v0.py:75-87: encoder prologue (pluggable) + `_call`."""
        if combined_features is None:
            b, v = inputs[2].shape[:2]
            feats = self.encode(self._dev(inputs[2]).reshape(b * v, *inputs[2].shape[2:]))
            combined_features = feats.reshape(b, v, *feats.shape[1:])
        return self._call(inputs, inputs[0].shape[1], inputs[0].shape[0], combined_features, **kw)

    __call__ = call

    @staticmethod
    def volumetric_render(zs, density, chromacity):
        """model_v0.py:89-100 -> (rgb, depth, weights)."""
        rgbs = torch.cat([chromacity, density[..., None]], dim=-1).contiguous()
        return ops.composite(zs.contiguous(), rgbs, return_weights=True)

    # ---- training (model_v0.py:186-197, train_nerf.py:20-34, nerf_utils.py:8-12) -----------------------------
    def compile(self, learning_rate=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-7, gradients_clip=1.0,
                train_readout=False, grad_sync=None, encoder_optimizer=None, deterministic=None):
        """train_nerf.py:20-34: MSE loss, Adam(1e-4) on the coarse and fine embeddings.
        `learning_rate` may be a callable of the step (e.g. nerf_utils.WarmupScheduler).
        train_readout=False mirrors the reference's MultiOptimizer list, which names only the two embeddings
        (SURVEY.md Q9); set True to update the RenderReadout kernels as well.
        grad_sync: optional callable on the single flat gradient buffer (494 600 fp32), e.g.
        distributed.allreduce_mean_ for data-parallel training (one collective per step).
        deterministic: kept for callers (ops.set_deterministic): the weight gradients are summed in a fixed order in any case.
        """
        if deterministic is not None:
            ops.set_deterministic(deterministic)
        self._opt = dict(lr=learning_rate, b1=beta_1, b2=beta_2, eps=epsilon, clip=gradients_clip, step=0)
        self._grad = torch.zeros(2 * NET_PARAMS, dtype=torch.float32, device=self.device)
        self._adam_m = torch.zeros_like(self._grad)
        self._adam_v = torch.zeros_like(self._grad)
        mask = torch.ones(NET_PARAMS, dtype=torch.uint8, device=self.device)
        if not train_readout:
            mask[_EMB_PARAMS:] = 0
        self._update_mask = torch.cat([mask, mask]).contiguous()
        self._grad_sync = grad_sync
        self._train_bufs = {}
        # optional torch optimizer over the parameters of `feature_encoder` (a torch.nn.Module): train_step then also
        # back-propagates dL/d(combined_features) into the encoder (used only when train_step encodes the images itself)
        self._encoder_optimizer = encoder_optimizer

    def loss_and_grads(self, inputs, labels, combined_features, u_coarse=None, u_fine=None, generator=None,
                       stop_fine_z=False, return_d_features=False):
        """Forward + backward of loss = MSE(labels, rgb) + MSE(labels, fine_rgb) (model_v0.py:190-194).
        Returns (loss 1-element device tensor, flat gradient (2 x 247300): [coarse | fine], outputs 4-tuple).
        Gradient scope: all MLP variables, including the path the reference leaves open (no stop_gradient on the
        importance samples): fine loss -> fine sample positions -> sample_pdf -> coarse weights ->
        coarse network.  stop_fine_z=True cuts that path (cheaper).
        return_d_features: also return dL/d(combined_features) (B,V,H,W,256) as a 4th element - the cotangent an
        upstream feature encoder (trained in the reference, train_nerf.py:27-32) continues from."""
        if not hasattr(self, '_grad'):
            self.compile()
        call, keep = self._train_call(inputs, labels, combined_features, u_coarse, u_fine, generator, stop_fine_z, return_d_features)
        # ONE C call: mvnerf_loss_and_grads (csrc/train_api.hip).  Its struct has no room for a per-call kernel choice, so the training
        # forward follows the process-wide value: it is set for the length of the call (the choice is read when the passes are
        # launched) and put back, so that one model's training does not choose another model's or caller's kernel
        prev = ops.set_split_kernel(self.f32_gemm) if keep['split'] is not None else None
        try:
            ops.loss_and_grads(call, keep['rays_o'])
        finally:
            if prev is not None:
                ops.set_split_kernel(prev)
        self._last_call = (call, keep)
        if return_d_features:
            return keep['loss'], self._grad, keep['outputs'], keep['d_features']
        return keep['loss'], self._grad, keep['outputs']

    def _train_call(self, inputs, labels, combined_features, u_coarse, u_fine, generator, stop_fine_z, return_d_features):
        """The mvnerf_train_call of one step: device tensors checked and bound, workspace and weight images cached per shape."""
        rays_o, rays_d, images, k4, einv = [self._dev(t) for t in inputs]
        feats = self._dev(combined_features)
        y = self._dev(labels)
        b, r, _ = rays_o.shape
        v, h, w = images.shape[1:4]
        u_coarse, u_fine = self._uniforms(b, r, u_coarse, u_fine, generator)
        u_coarse, u_fine = self._dev(u_coarse), self._dev(u_fine)
        pc, pf = self.packed()
        if self._packed_bwd is None:
            self._packed_bwd = (ops.pack_bwd_streams(self.coarse_net), ops.pack_bwd_streams(self.fine_net))
        # the training forward runs on the same split kernel as inference (loss_and_grads selects it); the backward's layer launches
        # always use fp16 two-piece products, which is why a training step has the tighter range of check_range(training=True)
        split = self.packed_split() if self.f32_gemm != 'mfma_f32' else None
        use_tables = ops.texel_table_pays(r, self.n_samples, h, w)      # layer 0's feature rows per texel
        tb = self._train_bufs
        key = (b, v, r, h, w, bool(return_d_features))
        if tb.get('key') != key:
            tb.clear()
            tb['key'] = key
            tb['workspace'] = torch.empty(ops.train_workspace_bytes(b, v, r, self.n_samples, h, w, use_tables, return_d_features),
                                          dtype=torch.uint8, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        outputs = (torch.empty((b, r, 3), dtype=torch.float32, device=self.device), torch.empty((b, r), dtype=torch.float32, device=self.device),
                   torch.empty((b, r, 3), dtype=torch.float32, device=self.device), torch.empty((b, r), dtype=torch.float32, device=self.device))
        d_feat = torch.empty_like(feats) if return_d_features else None
        keep = dict(rays_o=rays_o, rays_d=rays_d, images=images, feats=feats, k4=k4, einv=einv, u=(u_coarse, u_fine), y=y, loss=loss,
                    outputs=outputs, d_features=d_feat, packed=(pc, pf), split=split, bwd=self._packed_bwd)
        call = ops.train_call(rays_o, rays_d, images, feats, k4, einv, u_coarse, u_fine, y, self.near, self.far,
                              (self.coarse_net, self.fine_net), (pc, pf), split, self._packed_bwd, loss, self._grad, outputs, tb['workspace'],
                              q7_mode=self.q7_mode, stop_fine_z=stop_fine_z, use_tables=use_tables, d_features=d_feat)
        if hasattr(self._grad_sync, 'event_handle'):         # distributed.OverlappedGradSync: the fine half's all-reduce starts early
            call.fine_grad_event = self._grad_sync.event_handle()
        return call, keep

    def train_step(self, data, combined_features=None, u_coarse=None, u_fine=None, generator=None, stop_fine_z=False):
        """model_v0.py:186-197: one optimisation step on (inputs, labels); returns {'loss': 1-element tensor}."""
        inputs, labels = data
        enc_opt = getattr(self, '_encoder_optimizer', None)
        train_encoder = combined_features is None and enc_opt is not None
        if combined_features is None:
            bsz, v = inputs[2].shape[:2]
            with torch.set_grad_enabled(train_encoder):
                feats = self.encode(self._dev(inputs[2]).reshape(bsz * v, *inputs[2].shape[2:]))
                combined_features = feats.reshape(bsz, v, *feats.shape[1:])
        if train_encoder:
            # the reference's optimizer list also names the feature encoders (train_nerf.py:27-32): the HIP backward hands
            # dL/d(combined_features) back to torch autograd, which continues into the encoder's variables
            loss, grad, _, d_feat = self.loss_and_grads(inputs, labels, combined_features.detach().contiguous(), u_coarse, u_fine,
                                                        generator, stop_fine_z, return_d_features=True)
            enc_opt.zero_grad(set_to_none=True)
            combined_features.backward(d_feat.to(combined_features.dtype))
            if self._grad_sync is not None:              # data parallel: the encoder's gradients ride in ONE more flat collective
                grads = [prm.grad for group in enc_opt.param_groups for prm in group['params'] if prm.grad is not None]
                if grads:
                    flat = torch._utils._flatten_dense_tensors(grads)
                    self._grad_sync(flat)
                    for g_, f_ in zip(grads, torch._utils._unflatten_dense_tensors(flat, grads)):
                        g_.copy_(f_)
            for group in enc_opt.param_groups:           # optimize(): clip-by-value, then the optimizer step
                for prm in group['params']:
                    if prm.grad is not None:
                        prm.grad.clamp_(-self._opt['clip'], self._opt['clip'])
            enc_opt.step()
        else:
            loss, grad, _ = self.loss_and_grads(inputs, labels, combined_features, u_coarse, u_fine, generator, stop_fine_z)
        if self._grad_sync is not None:
            self._grad_sync(grad)                         # one flat collective for both MLPs
        self.apply_gradients(grad)
        return {'loss': loss}

    def apply_gradients(self, grad):
        """optimize() (nerf_utils.py:8-12) on the flat gradient [coarse | fine]: clip-by-value, Adam (tf.keras, eps 1e-7)."""
        o = self._opt
        # Keras evaluates the schedule at `optimizer.iterations` BEFORE the increment (0 on the first step: the warm-up's
        # first update has lr = 0); only the Adam bias correction uses iterations + 1
        lr = o['lr'](o['step']) if callable(o['lr']) else o['lr']
        o['step'] += 1
        lr_t = lr * np.sqrt(1.0 - o['b2'] ** o['step']) / (1.0 - o['b1'] ** o['step'])
        if grad.data_ptr() != self._grad.data_ptr():
            self._grad.copy_(grad)
        adam = ops.adam_state(self._adam_m, self._adam_v, lr_t, o['b1'], o['b2'], o['eps'], o['clip'], self._update_mask, repack=True)
        call = getattr(self, '_last_call', (None, None))[0]
        if call is None:                                     # gradients that did not come from loss_and_grads: only the variables move
            call = ops._lib.TrainCall()
            call.net_coarse, call.net_fine, call.grad = self.coarse_net.data_ptr(), self.fine_net.data_ptr(), self._grad.data_ptr()
            ops.apply_gradients(call, adam, self._grad)
            self.weights_changed()
            return
        # mvnerf_apply_gradients: clip + Adam on both MLPs, then the weight images of the call (packed, split, transposed streams) are
        # rebuilt in place - they are this model's cached ones, so they stay valid; the derived caches are dropped
        ops.apply_gradients(call, adam, self._grad)
        self._packed16 = None
        self._tables_key = None
        self._weight_range = None
        if not call.split_coarse:
            self._packed_split = None

    # ---- checkpoint (model_v0.py:199-240; per-sub-model files, load() -> False if any is missing) ----
    def _split(self, flat):
        return flat[:_EMB_PARAMS], flat[_EMB_PARAMS:]

    def _encoder_modules(self):
        """The sub-models of `feature_encoder` that have files of their own (model_v4.py:196-240), by file name."""
        enc = self.feature_encoder
        missing = [name for name in ENCODER_SUBMODELS if not isinstance(getattr(enc, name, None), torch.nn.Module)]
        if missing:
            raise ValueError(f'encoders=True: feature_encoder ({type(enc).__name__}) has no sub-module {missing[0]!r} '
                             '(expected e.g. an encoders.FeatureProducerV4)')
        return {name: getattr(enc, name) for name in ENCODER_SUBMODELS}

    def store(self, path, encoders=False):
        """The four MLP files; with encoders=True also `{path}_visual_features.pt` and `{path}_combine_clip_visual.pt`, the CPU state
        dicts of the feature encoder's sub-models - the six files of the reference's renderer, which `LanguageNeRF.load_backbone` reads."""
        modules = self._encoder_modules() if encoders else {}
        parts = dict(zip(_SUBMODELS, (*self._split(self.coarse_net), *self._split(self.fine_net))))
        for name, t in parts.items():
            torch.save(t.detach().cpu(), f'{path}_{name}.pt')
        for name, module in modules.items():
            torch.save({k: v.detach().cpu().clone() for k, v in module.state_dict().items()}, f'{path}_{name}.pt')

    def load(self, path, old=False, encoders=False):
        """-> True, or False (nothing changed) if any file is missing: the four MLP files, with encoders=True the two encoder files too."""
        modules = self._encoder_modules() if encoders else {}
        files = [f'{path}_{name}.pt' for name in _SUBMODELS]
        if not all(os.path.exists(f) for f in files + [f'{path}_{name}.pt' for name in modules]):
            return False
        ce, cr, fe, fr = [torch.load(f, weights_only=True) for f in files]
        states = {name: torch.load(f'{path}_{name}.pt', weights_only=True) for name in modules}
        for name, module in modules.items():                  # every key and shape before anything is written
            check_state_dict(module, states[name], f'{path}_{name}.pt')
        self.set_weights(torch.cat([ce, cr]), torch.cat([fe, fr]))
        for name, module in modules.items():
            module.load_state_dict(states[name])
        return True

    def _dev(self, t):
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
        return t.to(self.device, dtype=torch.float32).contiguous()


def camera_parameters(camera_config):
    """data_generator/util.py:4-10: (extrinsics_inv, intrinsics padded to 4x4), float64 NumPy."""
    k = np.reshape(camera_config['intrinsics'], (3, 3))
    k4 = np.concatenate((k, np.zeros((3, 1))), axis=1)
    k4 = np.concatenate((k4, np.array([[0, 0, 0, 1]])), axis=0)
    return np.linalg.inv(camera_config['pose']), k4


def render(rays, model, *, features, images, K4, Einv, near=None, far=None, n_samples=64, u_coarse=None, u_fine=None,
           generator=None, return_coarse=False):
    """render(rays, model) -> (rgb, depth): the fine pair by default, the reference 4-tuple
    (rgb, depth, fine_rgb, fine_depth) (model_v0.py:184) with return_coarse=True.
    rays = (origins (B,R,3), directions (B,R,3))."""
    if n_samples != model.n_samples:
        raise ValueError(f'n_samples={n_samples} but the model was built with {model.n_samples}')
    saved = model.near, model.far
    if near is not None:
        model.near = near
    if far is not None:
        model.far = far
    try:
        out = model._call((rays[0], rays[1], images, K4, Einv), rays[0].shape[1], rays[0].shape[0], features,
                          u_coarse=u_coarse, u_fine=u_fine, generator=generator)
    finally:
        model.near, model.far = saved
    return out if return_coarse else (out[2], out[3])


def render_view(model, src_colors, src_camera_configs, tgt_camera_config, combined_features=None, generator=None,
                chunk=None, range_check=False):
    """model_v0.py:243-281.  src_colors: list of (H,W,>=3) uint8 images; camera configs: dicts with
    'pose' (4x4) and 'intrinsics' (9,).  Returns (rgb (H,W,3) uint8, depth (H,W,1) uint8) as NumPy.
    Everything between the upload of the source views and the download of the two uint8 images stays on
    the device; `chunk` rays per `_call` (default: the whole image in one call).
    range_check: render on the range-guarded split_f16 kernel; the status is zeroed before the frame and read ONCE behind its last
    chunk (one host synchronisation per frame).  Out of range the frame is rendered again on 'split_bf16' with a RuntimeWarning
    (range_policy='fallback') or FloatingPointError is raised ('raise')."""
    dev = model.device
    tgt_k = np.reshape(tgt_camera_config['intrinsics'], (3, 3)).astype(np.float32)
    h, w = src_colors[0].shape[:2]
    pose = np.asarray(tgt_camera_config['pose'], dtype=np.float64)
    m = pose[:3, :3] @ np.linalg.inv(tgt_k[:3, :3])                      # nerf_utils.py:30, host LAPACK as the reference
    rays_o, rays_d = ops.get_rays_device(m, pose[:3, 3], dev, width=w, height=h)
    src = np.array([[img[..., :3] / 255.0 for img in src_colors]])         # (1,V,H,W,3), model_v0.py:253
    images = torch.from_numpy(src.astype(np.float32)).to(dev)
    cams = [camera_parameters(c) for c in src_camera_configs]              # data_generator/mvnerf.py:28-43
    einv = torch.from_numpy(np.array([[c[0] for c in cams]], dtype=np.float32)).to(dev)
    k4 = torch.from_numpy(np.array([[c[1] for c in cams]], dtype=np.float32)).to(dev)
    if combined_features is None:
        feats = model.encode(images.reshape(-1, h, w, 3))
        combined_features = feats.reshape(1, len(src_colors), *feats.shape[1:])
    n = h * w
    chunk = n if chunk is None else int(chunk)
    rgbs = torch.empty((n, 3), dtype=torch.float32, device=dev)
    depths = torch.empty((n,), dtype=torch.float32, device=dev)
    frame = object() if model.compute_dtype == 'f32' else None           # texel tables: built by the first chunk, then re-used

    def render_chunks(**kw):
        if frame is not None:
            kw['scene_key'] = frame
        for i in range(0, n, chunk):
            sl = slice(i, min(n, i + chunk))
            out = model.infer((rays_o[None, sl], rays_d[None, sl], images, k4, einv), combined_features, generator=generator, **kw)
            rgbs[sl], depths[sl] = out[2][0], out[3][0]

    guarded = bool(range_check) and model.compute_dtype == 'f32' and model.f32_gemm == 'split_f16' and model.range_policy != 'off'
    if guarded:
        model.range_reset()
        # (a fallback frame draws the same uniforms as the frame it replaces)
        rng_state = generator.get_state() if generator is not None else torch.cuda.get_rng_state(dev)
        render_chunks(range_check=True)
        rep = model.range_report()                                        # the frame's one host read
        max_a = rp.worst([rep['coarse']['max_activation'], rep['fine']['max_activation']])
        # (the weights have been dealt with by the calls themselves: out of range they already ran on 'split_bf16', which leaves the status at 0)
        action = rp.decide(model.range_policy, model.f32_gemm, max_activation=max_a)
        if action == rp.RAISE:
            raise FloatingPointError(rp.describe(None, max_a))
        if action == rp.FALLBACK:
            warnings.warn(rp.describe(None, max_a) + " - rendering the frame again on 'split_bf16'", RuntimeWarning, stacklevel=2)
            if generator is not None:
                generator.set_state(rng_state)
            else:
                torch.cuda.set_rng_state(rng_state, dev)
            render_chunks(kernel='split_bf16')
    else:
        render_chunks()
    rgb8, depth8 = ops.finish_view(rgbs, depths)
    return rgb8.reshape(h, w, 3).cpu().numpy(), depth8.reshape(h, w, 1).cpu().numpy()
