"""LanguageNeRF.compile(fused_optimizer=True): the read-out's optimiser and the whole training step behind the C ABI (csrc/language_opt.hip:
mvnerf_language_apply_gradients, mvnerf_language_train_step), on the GPU.

The yardstick of the update is the kernel the other two optimisers of this project already use, mvnerf_adam_clip, called once per variable
with the rate of tests/language_adam_ref.py::rate32: every comparison with it is bit for bit.  The whole step is held to the fill protocol
of tests/step_chains.py against the chain of its parts (stack, mvnerf_language_loss_and_grads, 21 x mvnerf_adam_clip); the Python path to
the bits of that chain and to the float64 reference under the bar tests/test_language_adam_cpu.py derives; the captured graph to an eager
twin; the kept trunk images to a fresh model.  Small cases of tests/test_gpu_language_step.py throughout."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import language_adam_ref as A
from tests import step_chains as S
from tests.test_gpu_language_step import CASES, case, run_step
from thesis_clip_nerf_amd import _lib, ops
from thesis_clip_nerf_amd import lmvnerf as M
from thesis_clip_nerf_amd import train_language as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 12345.0
HEAD = ('w4', 'b4')
LR = 1e-3
N_STEPS = 3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return torch.equal(S.bits(a), S.bits(b))


# ---- 1. the update alone ------------------------------------------------------------------------------------------------------------------
def guarded(values):
    """values (any shape) with one guard word in front and behind -> (whole, inner view of values' shape).  The inner view starts 4 bytes
    into the allocation: no variable here is 16-byte aligned."""
    whole = torch.full((values.numel() + 2,), GUARD, dtype=torch.float32, device=DEV)
    whole[1:-1] = values.reshape(-1).to(DEV)
    return whole, whole[1:-1].view(values.shape)


def guards_hold(whole):
    return float(whole[0]) == GUARD and float(whole[-1]) == GUARD


def segments(n5):
    """(name, part or None, begin, count, shape) of the 21 variables in flat order."""
    out = []
    for name, (offset, shape) in A.layout(n5)[0].items():
        if name in HEAD:
            each = int(np.prod(shape[1:]))
            out += [(name, k, offset + k * each, each, shape[1:]) for k in range(4)]
        else:
            out.append((name, None, offset, int(np.prod(shape)), shape))
    return out


class Update:
    """One mvnerf_language_apply_gradients problem on caller-owned, guarded buffers: the 21 variables as separate tensors, m / v / grads
    flat, the counter, and NaN-filled stacked head images."""

    def __init__(self, n5, counter, seed, grads=None, zero_moments=False):
        self.n5, self.segs = n5, segments(n5)
        self.total = A.layout(n5)[1]
        rng = np.random.default_rng(seed)
        f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))
        self.vars = [guarded(f32(0.1 * rng.standard_normal(shape))) for _, _, _, _, shape in self.segs]
        g = 0.8 * rng.standard_normal(self.total)                                      # a fifth of them beyond the clip
        self.grads = guarded(f32(g if grads is None else grads))
        self.m = guarded(f32(np.zeros(self.total) if zero_moments else 0.05 * rng.standard_normal(self.total)))
        self.v = guarded(f32(np.zeros(self.total) if zero_moments else rng.uniform(0.0, 0.05, self.total)))
        self.w4 = guarded(torch.full((4, 64, 128), float('nan')))
        self.b4 = guarded(torch.full((4, 64), float('nan')))
        self.step = torch.tensor([-7, counter, -7], dtype=torch.int64, device=DEV)

    def tensor(self, name, part=None):
        return next(v[1] for v, s in zip(self.vars, self.segs) if s[0] == name and s[1] == part)

    def structs(self, hyper):
        c = _lib.LanguageCall()
        c.grads, c.n5 = self.grads[1].data_ptr(), self.n5
        a = _lib.LanguageAdam()
        for k in range(4):
            a.head_w[k], a.head_b[k] = self.tensor('w4', k).data_ptr(), self.tensor('b4', k).data_ptr()
        a.head_wc, a.head_bc = self.tensor('wc').data_ptr(), self.tensor('bc').data_ptr()
        for i, name in enumerate(A.TAIL_ORDER):
            a.tail_w[i] = self.tensor(name).data_ptr()
        a.head_w4, a.head_b4 = self.w4[1].data_ptr(), self.b4[1].data_ptr()
        a.m, a.v, a.step = self.m[1].data_ptr(), self.v[1].data_ptr(), self.step[1:].data_ptr()
        a.lr, a.beta1, a.beta2, a.eps, a.clip = (hyper[k] for k in ('lr', 'beta1', 'beta2', 'eps', 'clip'))
        return c, a

    def apply(self, hyper):
        c, a = self.structs(hyper)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = _lib.lib().mvnerf_language_apply_gradients(ctypes.byref(c), ctypes.byref(a), stream)
        assert rc == 0, _lib.lib().mvnerf_last_error()
        torch.cuda.synchronize()

    def yardstick(self, hyper, counter):
        """21 calls of mvnerf_adam_clip on copies -> (variables, m, v)."""
        lr_t = float(A.rate32(hyper['lr'], hyper['beta1'], hyper['beta2'], counter + 1))
        m, v = self.m[1].clone(), self.v[1].clone()
        out = []
        for (whole, inner), (_, _, begin, count, _) in zip(self.vars, self.segs):
            p = inner.clone().reshape(-1)
            S.call('mvnerf_adam_clip', p, self.grads[1][begin:], m[begin:], v[begin:], count, lr_t, hyper['beta1'], hyper['beta2'], hyper['eps'],
                   hyper['clip'], None)
            out.append(p.view(inner.shape))
        torch.cuda.synchronize()
        return out, m, v

    def check(self, want, counter):
        want_vars, want_m, want_v = want
        for (whole, inner), w, seg in zip(self.vars, want_vars, self.segs):
            assert guards_hold(whole), seg[:2]
            assert same_bits(inner, w), seg[:2]
        for name, (whole, inner), w in (('m', self.m, want_m), ('v', self.v, want_v)):
            assert guards_hold(whole) and same_bits(inner, w), name
        assert guards_hold(self.grads[0]) and guards_hold(self.w4[0]) and guards_hold(self.b4[0])
        assert self.step.tolist() == [-7, counter + 1, -7]
        assert same_bits(self.w4[1], torch.stack([self.tensor('w4', k) for k in range(4)]))
        assert same_bits(self.b4[1], torch.stack([self.tensor('b4', k) for k in range(4)]))


@pytest.mark.parametrize('clip', (1.0, 0.0))
@pytest.mark.parametrize('counter', (0, 1, 9, 999))
@pytest.mark.parametrize('n5', (1, 7))
def test_update_alone_has_the_bits_of_adam_clip_per_variable(n5, counter, clip):
    hyper = dict(A.HYPER, clip=clip)
    u = Update(n5, counter, seed=10 * n5 + counter)
    assert u.total % 2 == 1 and float((u.grads[1].abs() > 1.0).float().mean()) > 0.1
    want = u.yardstick(hyper, counter)
    before = [inner.clone() for _, inner in u.vars]
    u.apply(hyper)
    u.check(want, counter)
    assert all(not same_bits(a, inner) for a, (_, inner) in zip(before, u.vars))       # every variable moved


@pytest.mark.parametrize('clip', (1.0, 0.0))
def test_one_nan_gradient_reaches_exactly_its_own_element(clip):
    """clip = 0: NaN in p, m, v of that element; clip = 1: fmaxf(NaN, -clip) = -clip, as in mvnerf_adam_clip.  Nothing else changes."""
    hyper = dict(A.HYPER, clip=clip)
    n5, counter = 1, 1
    probe = Update(n5, counter, seed=5)
    begin = next(s for s in probe.segs if s[0] == 'w1b')[2]
    at = begin + 77
    base = probe.grads[1].cpu().numpy().copy()
    base[at] = 0.25                                              # inside the clip: the NaN's -clip is another value
    clean = Update(n5, counter, seed=5, grads=base)
    grads = base.copy()
    grads[at] = np.nan
    dirty = Update(n5, counter, seed=5, grads=grads)
    want = dirty.yardstick(hyper, counter)
    clean.apply(hyper)
    dirty.apply(hyper)
    dirty.check(want, counter)
    for (_, a), (_, b), seg in zip(clean.vars, dirty.vars, dirty.segs):
        differ = (S.bits(a) != S.bits(b)).reshape(-1).nonzero().reshape(-1).tolist()
        assert differ == ([77] if seg[0] == 'w1b' else []), seg[:2]
    for a, b in ((clean.m[1], dirty.m[1]), (clean.v[1], dirty.v[1])):
        assert (S.bits(a) != S.bits(b)).nonzero().reshape(-1).tolist() == [at]
    p = dirty.tensor('w1b').reshape(-1)[77]
    assert bool(torch.isnan(p)) == (clip == 0.0) and bool(torch.isnan(dirty.m[1][at])) == (clip == 0.0)


def test_zero_gradients_on_zero_moments_leave_the_variables_untouched():
    u = Update(7, 0, seed=3, grads=np.zeros(A.layout(7)[1]), zero_moments=True)
    before = [inner.clone() for _, inner in u.vars]
    u.apply(A.HYPER)
    assert all(same_bits(a, inner) for a, (_, inner) in zip(before, u.vars))
    assert not u.m[1].any() and not u.v[1].any() and u.step.tolist() == [-7, 1, -7]
    assert same_bits(u.w4[1], torch.stack([u.tensor('w4', k) for k in range(4)]))


# ---- 2. the whole step through ctypes only -------------------------------------------------------------------------------------------------
def moved_poses(inputs, steps=N_STEPS, seed=3):
    rng = np.random.default_rng(seed)
    return [tuple((a + 0.02 * rng.standard_normal(a.shape)).astype(np.float32) for a in inputs[:4]) + tuple(inputs[4:]) for _ in range(steps)]


def initial_variables(model):
    """name -> tensor (clone) of the read-out of `model` by the names of the flat layout; w4 / b4 stacked."""
    heads, comb, tail = model._readout_tensors()
    out = {'w4': torch.stack([lin.weight.detach() for lin in heads]), 'b4': torch.stack([lin.bias.detach() for lin in heads]),
           'wc': comb.weight.detach().clone(), 'bc': comb.bias.detach().clone()}
    out.update({k: t.detach().clone() for k, t in tail.items()})
    return out


def problem(name):
    """The scene of a case on the device, the trunk's images, the read-out's initial variables and the moving poses."""
    n_views, batch, n_points, representation = CASES[name]
    sc, inputs, labels, model = case(name)
    state = model.trunk_state(inputs, sc['features'])
    return dict(name=name, B=batch, V=n_views, np=n_points, n5=model.n_transforms_to_check, rep=0 if representation == 'quaternion' else 1,
                H=sc['images'].shape[2], W=sc['images'].shape[3], state=state, offsets=model.transforms_to_check.clone(),
                variables=initial_variables(model), labels=[dev(a) for a in labels],
                poses=[[dev(a) for a in moved[:4]] for moved in moved_poses(inputs)])


def fill_call(pr, variables, w4, b4, poses, grads, prediction, scalars, workspace):
    """A mvnerf_language_call filled field by field from raw pointers."""
    c = _lib.LanguageCall()
    st = pr['state']
    c.images, c.features, c.intrinsics, c.extrinsics_inv = (t.data_ptr() for t in st.geo)
    c.B, c.V, c.H, c.W = pr['B'], pr['V'], pr['H'], pr['W']
    c.packed_net, c.split, c.bwd_streams = st.packed.data_ptr(), st.packed_split.data_ptr(), st.bwd_streams.data_ptr()
    c.head_w4, c.head_b4, c.head_wc, c.head_bc = w4.data_ptr(), b4.data_ptr(), variables['wc'].data_ptr(), variables['bc'].data_ptr()
    for i, k in enumerate(A.TAIL_ORDER):
        c.tail_w[i] = variables[k].data_ptr()
    c.offsets = pr['offsets'].data_ptr()
    c.rep, c.np, c.n5 = pr['rep'], pr['np'], pr['n5']
    c.t_landscape, c.rot_landscape, c.t_grad, c.rot_grad = (t.data_ptr() for t in poses)
    c.label_landscape, c.label_grad_t, c.label_grad_r = (t.data_ptr() for t in pr['labels'])
    c.loss_kind, c.w_land, c.w_t, c.w_r = 0, 1.0, 1.0, 1.0
    c.grads, c.prediction, c.scalars = grads.data_ptr(), prediction.data_ptr(), scalars.data_ptr()
    c.workspace, c.workspace_bytes = workspace.data_ptr(), workspace.numel()
    return c


def step_buffers(fill, pr):
    """Everything a step writes, from `fill`: the 21 variables (w4 / b4 as the four layers each, separate tensors), moments, the counter,
    the stacked images, the step's outputs."""
    total = A.layout(pr['n5'])[1]
    variables = {k: fill(tuple(v.shape), name=k, init=v) for k, v in pr['variables'].items() if k not in HEAD}
    heads_w = [fill((64, 128), name=f'head_w[{k}]', init=pr['variables']['w4'][k]) for k in range(4)]
    heads_b = [fill((64,), name=f'head_b[{k}]', init=pr['variables']['b4'][k]) for k in range(4)]
    zeros = torch.zeros(total, device=DEV)
    return dict(variables=variables, heads_w=heads_w, heads_b=heads_b, m=fill((total,), name='m', init=zeros), v=fill((total,), name='v', init=zeros),
                step=fill((2,), dtype=torch.int32, name='step', init=torch.zeros(2, dtype=torch.int32, device=DEV)),
                w4=fill((4, 64, 128), name='head_w4'), b4=fill((4, 64), name='head_b4'), grads=fill((total,), name='grads'),
                prediction=fill((pr['B'], pr['np']), name='prediction'), scalars=fill((4,), name='scalars'))


def outputs(b):
    out = dict(b['variables'])
    out.update({f'head_w{k}': t for k, t in enumerate(b['heads_w'])})
    out.update({f'head_b{k}': t for k, t in enumerate(b['heads_b'])})
    out.update({k: b[k] for k in ('m', 'v', 'step', 'w4', 'b4', 'grads', 'prediction', 'scalars')})
    return out


def workspace_bytes(pr):
    return S.size('mvnerf_language_workspace_bytes', pr['B'], pr['V'], pr['H'], pr['W'], pr['np'], pr['n5'])


def c_step(fill, pr, steps=N_STEPS, trace=None):
    """mvnerf_language_train_step, `steps` times on moving poses, through ctypes alone."""
    b = step_buffers(fill, pr)
    ws = fill(workspace_bytes(pr), name='workspace')
    a = _lib.LanguageAdam()
    for k in range(4):
        a.head_w[k], a.head_b[k] = b['heads_w'][k].data_ptr(), b['heads_b'][k].data_ptr()
    a.head_wc, a.head_bc = b['variables']['wc'].data_ptr(), b['variables']['bc'].data_ptr()
    for i, k in enumerate(A.TAIL_ORDER):
        a.tail_w[i] = b['variables'][k].data_ptr()
    a.head_w4, a.head_b4, a.m, a.v, a.step = (b[k].data_ptr() for k in ('w4', 'b4', 'm', 'v', 'step'))
    a.lr, a.beta1, a.beta2, a.eps, a.clip = LR, A.HYPER['beta1'], A.HYPER['beta2'], A.HYPER['eps'], A.HYPER['clip']
    lib = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for poses in pr['poses'][:steps]:
        c = fill_call(pr, b['variables'], b['w4'], b['b4'], poses, b['grads'], b['prediction'], b['scalars'], ws)
        assert lib.mvnerf_language_train_step(ctypes.byref(c), ctypes.byref(a), stream) == 0, lib.mvnerf_last_error()
        if trace is not None:
            torch.cuda.synchronize()
            trace.append({k: v.clone() for k, v in outputs(b).items()})
    return outputs(b)


def chain(fill, pr, steps=N_STEPS, trace=None):
    """The step by hand: stack, mvnerf_language_loss_and_grads, 21 x mvnerf_adam_clip at the restated rate, the images re-stacked, the
    counter advanced."""
    b = step_buffers(fill, pr)
    segs = segments(pr['n5'])
    lib = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = A.HYPER
    for counter, poses in enumerate(pr['poses'][:steps]):
        b['w4'].copy_(torch.stack(b['heads_w']))
        b['b4'].copy_(torch.stack(b['heads_b']))
        ws = fill(workspace_bytes(pr), name='workspace')
        c = fill_call(pr, b['variables'], b['w4'], b['b4'], poses, b['grads'], b['prediction'], b['scalars'], ws)
        assert lib.mvnerf_language_loss_and_grads(ctypes.byref(c), stream) == 0, lib.mvnerf_last_error()
        lr_t = float(A.rate32(LR, h['beta1'], h['beta2'], counter + 1))
        for name, part, begin, count, _ in segs:
            p = b['variables'][name] if part is None else (b['heads_w'] if name == 'w4' else b['heads_b'])[part]
            S.call('mvnerf_adam_clip', p, b['grads'][begin:], b['m'][begin:], b['v'][begin:], count, lr_t, h['beta1'], h['beta2'], h['eps'],
                   h['clip'], None)
        b['w4'].copy_(torch.stack(b['heads_w']))
        b['b4'].copy_(torch.stack(b['heads_b']))
        b['step'][0] = counter + 1
        if trace is not None:
            torch.cuda.synchronize()
            trace.append({k: v.clone() for k, v in outputs(b).items()})
    return outputs(b)


@functools.lru_cache(maxsize=None)
def chain_trace(name):
    """The chain's buffers after every step, once per case (zero fill)."""
    trace = []
    chain(S.Fill(0, DEV), problem(name), trace=trace)
    return trace


@pytest.mark.parametrize('name', ['v1b2p3_q', 'v1b1p1_6d'])
def test_whole_step_through_ctypes_alone_equals_the_chain_of_its_parts(name):
    """Three steps on moving poses at V = 1 (no unordered sum anywhere) under the fill protocol: a workspace of exactly
    mvnerf_language_workspace_bytes with a 4 KiB tail, every output and state buffer guarded, three fill words."""
    pr = problem(name)
    runs = S.run_fills(lambda fill: c_step(fill, pr), DEV, sync=torch.cuda.synchronize)
    want = chain_trace(name)[-1]
    assert want['step'].tolist() == [N_STEPS, 0]
    S.check_protocol(runs, want=want)
    moved = [k for k in pr['variables'] if k not in HEAD and not same_bits(want[k], pr['variables'][k])]
    assert len(moved) >= 11 and 'w0' in moved and 'wc' in moved, moved      # (one pose: the landscape term and two of its biases' gradients are zero)


# ---- 3. the Python path ---------------------------------------------------------------------------------------------------------------------
def model_variables(model):
    v = initial_variables(model)
    out = {k: t for k, t in v.items() if k not in HEAD}
    out.update({f'head_w{k}': v['w4'][k] for k in range(4)})
    out.update({f'head_b{k}': v['b4'][k] for k in range(4)})
    return out


@pytest.mark.parametrize('name', ['v1b2p3_q', 'v1b1p1_6d'])
def test_python_path_has_the_bits_of_the_ctypes_step_and_meets_float64(name):
    sc, inputs, labels, model = case(name)
    torch_twin = case(name)[3]
    model.compile(loss=M.kl_divergence, learning_rate=LR, fused_step=True, fused_optimizer=True)
    torch_twin.compile(loss=M.kl_divergence, learning_rate=LR, fused_step=True)
    assert model.optimizer is None and model.optimizer_steps() == 0
    n5 = model.n_transforms_to_check
    start = {k: v.cpu().numpy() for k, v in initial_variables(model).items()}
    params = list(model.grasp_readout.parameters())
    trace = chain_trace(name)
    for step, moved in enumerate(moved_poses(inputs)):
        out = model.train_step((moved, labels), sc['features'])
        out_torch = torch_twin.train_step((moved, labels), sc['features'])
        torch.cuda.synchronize()
        want = trace[step]
        for k, t in model_variables(model).items():
            assert same_bits(t, want[k]), (step, k)
        got = torch.stack([out[k] for k in ('landscape_loss', 'grad_loss_t', 'grad_loss_r', 'pred')])
        assert same_bits(got, want['scalars']) and same_bits(model._fs['grads'], want['grads'])
        assert same_bits(model._opt['m'], want['m']) and same_bits(model._opt['v'], want['v'])
        assert model.optimizer_steps() == step + 1
        assert all(p.grad is not None and p.grad.data_ptr() >= model._fs['grads'].data_ptr() for p in params)    # views of the flat gradient
        worst = max(float((a - b).detach().abs().max()) for a, b in zip(model.grasp_readout.parameters(), torch_twin.grasp_readout.parameters()))
        print(f'{name} step {step + 1}: max |fused optimizer - torch Adam| over the parameters {worst:.3e} (the formulas differ, DESIGN.md 10)')
        if step == 0:                                            # float64 of the whole update from this step's own gradient
            grads = model._fs['grads'].cpu().numpy()
            total = grads.size
            ref, _, _, bar = A.step64(start, grads, np.zeros(total, np.float32), np.zeros(total, np.float32), 0, n5, dict(A.HYPER, lr=LR))
            now = {k: v.cpu().numpy().astype(np.float64) for k, v in initial_variables(model).items()}
            for k in ref:
                err = np.abs(now[k] - ref[k])
                print(f'{name} {k}: worst |p - float64| / bar = {float((err / bar["p"][k]).max()):.3f}')
                assert (err <= bar['p'][k]).all(), k
    assert all(isinstance(p, torch.nn.Parameter) for p in params) and params == list(model.grasp_readout.parameters())


# ---- 4. graph replay ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,exact', [('v1b2p3_q', True), ('v2b2p3_6d', False)])
def test_graph_replay_matches_an_eager_twin(name, exact, tmp_path):
    """compile(graph=True, fused_optimizer=True) at lr = 1e-3: two eager steps, the capture, replays, against a twin stepping eagerly.  The
    rate changes with every step (t = 1 .. 5: 0.316 lr .. 0.173 lr), so a rate baked into the capture at step 3 shows at step 4.  V = 1:
    parameters and losses bit for bit.  V = 2: the losses to 1e-5, the bar of
    tests/test_gpu_language_step.py::test_fused_step_graph_replay_matches_eager (mvnerf_query_vjp's view sum uses atomics); the parameters'
    difference is printed.  Then load() between two replays: the next replay runs on the loaded read-out and trunk."""
    steps = 5
    sc, inputs, labels, eager = case(name)
    graphed = case(name)[3]
    rng = np.random.default_rng(7)
    datas = [((*[(a + 0.05 * rng.standard_normal(a.shape)).astype(np.float32) for a in inputs[:4]], *inputs[4:]), labels) for _ in range(steps + 1)]
    eager.compile(loss=M.kl_divergence, learning_rate=LR, fused_step=True, fused_optimizer=True)
    graphed.compile(loss=M.kl_divergence, learning_rate=LR, graph=True, fused_step=True, fused_optimizer=True)
    assert graphed.optimizer is None and eager.optimizer is None

    def compare(step, out_e, out_g):
        for k in out_e:
            a, b = float(out_e[k]), float(out_g[k])
            assert np.isfinite(a) and (a == b if exact else abs(a - b) < 1e-5 * max(1.0, abs(a))), (step, k, a, b)
        worst = 0.0
        for (n, a), (_, b) in zip(eager.grasp_readout.named_parameters(), graphed.grasp_readout.named_parameters()):
            if exact:
                assert same_bits(a, b), (step, n)
            worst = max(worst, float((a - b).detach().abs().max()))
        print(f'{name} step {step}: max |eager - replay| over the parameters {worst:.3e}')

    for step, data in enumerate(datas[:steps]):
        out_e = eager.train_step(data, sc['features'])
        out_g = graphed.train_step(data, sc['features'])
        torch.cuda.synchronize()
        compare(step, out_e, out_g)
    assert graphed._graph is not None
    assert graphed.optimizer_steps() == eager.optimizer_steps() == steps
    captured = graphed._graph
    other = case('v2b2p3_6d' if name == 'v1b2p3_q' else 'v1b1p1_6d')[3]      # the other seed: another trunk, another read-out
    path = str(tmp_path / 'other')
    other.store(path)
    before = [p.detach().clone() for p in graphed.grasp_readout.parameters()]
    assert graphed.load(path) and eager.load(path)
    assert not all(torch.equal(a, b) for a, b in zip(before, graphed.grasp_readout.parameters()))
    out_e = eager.train_step(datas[steps], sc['features'])
    out_g = graphed.train_step(datas[steps], sc['features'])
    torch.cuda.synchronize()
    assert graphed._graph is captured                             # a replay, not a new capture
    compare(steps, out_e, out_g)
    fresh = case(name)[3]
    fresh.compile(loss=M.kl_divergence, learning_rate=LR, fused_step=True)
    assert fresh.load(path)
    want, _ = fresh.loss_and_grads(datas[steps], sc['features'])
    for k in want:                                                # the losses of that replay are those of the loaded model
        a, b = float(want[k]), float(out_g[k])
        assert (a == b if exact else abs(a - b) < 1e-5 * max(1.0, abs(a))), (k, a, b)
    graphed.set_fused_optimizer(False)                            # a change of the flag drops the captured graph
    assert graphed._graph is None and isinstance(graphed.optimizer, torch.optim.Adam)


# ---- 5. the kept trunk images ---------------------------------------------------------------------------------------------------------------
def fresh_model(name, trunk_net, **flags):
    n_views, batch, n_points, representation = CASES[name]
    torch.manual_seed(50 + n_views)                               # the seed rule of case(): the same read-out
    model = M.LanguageNeRF(trunk_net, n_points_train=n_points, n_views=n_views, batch_size=batch, rotation_representation=representation,
                           softmax_before_loss=True, device=DEV)
    model.compile(loss=M.kl_divergence, **flags)
    return model


def step_outputs(model, data, features):
    out = model.train_step(data, features)
    torch.cuda.synchronize()
    return torch.stack([out[k] for k in ('landscape_loss', 'grad_loss_t', 'grad_loss_r', 'pred')]), model._fs['grads'].clone(), \
        model._fs['prediction'].clone()


def test_trunk_images_are_kept_across_steps_and_follow_the_trunk(tmp_path):
    name = 'v1b2p3_q'
    sc, inputs, labels, model = case(name)
    data = (inputs, labels)
    flags = dict(learning_rate=0.0, fused_step=True, fused_optimizer=True)     # lr = 0: every step sees the same read-out
    model.compile(loss=M.kl_divergence, **flags)
    first = step_outputs(model, data, sc['features'])
    kept = model._trunk_images['images']
    pointers = [t.data_ptr() for t in kept]
    cached = step_outputs(model, data, sc['features'])
    assert model._trunk_images['images'] is kept and model.trunk_state(inputs, sc['features']).packed_split is kept[1]
    fresh = step_outputs(fresh_model(name, sc['fine'], **flags), data, sc['features'])
    for a, b, c in zip(first, cached, fresh):
        assert same_bits(a, b) and same_bits(b, c)
    # the default path packs every step: new tensors
    plain = fresh_model(name, sc['fine'], learning_rate=0.0, fused_step=True)
    one, two = plain.trunk_state(inputs, sc['features']), plain.trunk_state(inputs, sc['features'])
    assert plain._trunk_images is None and one.packed is not two.packed and one.packed.data_ptr() != two.packed.data_ptr()
    # load_backbone of other weights: a new version -> packed again into the same buffers; the losses are a fresh model's on that trunk
    other_net = case('v2b2p3_6d')[0]['fine']
    assert not np.array_equal(other_net, sc['fine'])
    path = str(tmp_path / 'backbone')
    M.store_trunk(path, torch.from_numpy(np.ascontiguousarray(other_net)))
    assert model.load_backbone(path)
    loaded = step_outputs(model, data, sc['features'])
    assert [t.data_ptr() for t in model._trunk_images['images']] == pointers
    want = step_outputs(fresh_model(name, other_net, **flags), data, sc['features'])
    assert not same_bits(loaded[0], cached[0])
    for a, b in zip(loaded, want):
        assert same_bits(a, b)
    # a write through a raw pointer bumps no version: seen only after invalidate_trunk()
    zeros = torch.zeros_like(model.trunk_net)
    S.call('mvnerf_adam_clip', model.trunk_net, torch.full_like(model.trunk_net, 1.0), zeros, zeros.clone(), model.trunk_net.numel(), 1e-2, 0.9,
           0.999, 1e-7, 0.0, None)
    torch.cuda.synchronize()
    stale = step_outputs(model, data, sc['features'])
    for a, b in zip(stale, loaded):
        assert same_bits(a, b)
    model.invalidate_trunk()
    seen = step_outputs(model, data, sc['features'])
    want = step_outputs(fresh_model(name, model.trunk_net.cpu().numpy(), **flags), data, sc['features'])
    assert not same_bits(seen[0], stale[0])
    for a, b in zip(seen, want):
        assert same_bits(a, b)
    assert [t.data_ptr() for t in model._trunk_images['images']] == pointers


# ---- 6. the switch off, and the training loop ---------------------------------------------------------------------------------------------
def test_fused_optimizer_off_gives_the_bits_it_gave_before():
    """After tests/test_gpu_language_step.py::test_fused_step_off_gives_the_bits_it_gave_before: a model that took a step (at lr = 0) with
    the switch on and was switched back gives the bits of an untouched one, in loss_and_grads and in a step of torch's Adam."""
    name = 'v1b2p3_q'
    sc, inputs, labels, untouched = case(name)
    toggled = case(name)[3]
    assert untouched.fused_optimizer is False and toggled.fused_optimizer is False
    before = run_step(untouched, sc, inputs, labels, 'kl_divergence')
    toggled.compile(loss=M.kl_divergence, learning_rate=0.0, fused_step=True, fused_optimizer=True)
    toggled.train_step((inputs, labels), sc['features'])
    assert toggled.optimizer is None and toggled.optimizer_steps() == 1
    after = run_step(toggled, sc, inputs, labels, 'kl_divergence', fused_step=False, fused_optimizer=False)
    assert toggled.fused_optimizer is False and toggled._opt is None and toggled._trunk_images is None
    assert isinstance(toggled.optimizer, torch.optim.Adam)
    assert before[0] == after[0]
    np.testing.assert_array_equal(before[1], after[1])
    for k in before[2]:
        np.testing.assert_array_equal(before[2][k], after[2][k])
    for model in (untouched, toggled):
        model.compile(loss=M.kl_divergence, learning_rate=LR)
        model.train_step((inputs, labels), sc['features'])
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(untouched.grasp_readout.named_parameters(), toggled.grasp_readout.named_parameters()):
        assert same_bits(a, b), n


def test_train_language_with_fused_optimizer_learns(tmp_path, capsys):
    """train_language --fused-optimizer (which implies --fused-step) on the synthetic set, two epochs: the run completes with its files
    and the epoch mean of the landscape loss falls."""
    run, backbone = str(tmp_path / 'run'), str(tmp_path / 'backbone')
    np.random.seed(0)
    torch.manual_seed(0)
    T.main(['--model-path', run, '--backbone-path', backbone, '--init-backbone', '--epochs', '2', '--eval-after', '1', '--batch-size', '2',
            '--learning-rate', '1e-3', '--pose-augmentation-factor', '2', '--n-scenes', '8', '--n-perspectives', '3', '--n-initial-guesses', '64',
            '--n-optimization-steps', '2', '--valid-samples', '0', '1', '--fused-optimizer'])
    text = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r'Epoch \d+/\d+ - landscape_loss: ([-+0-9.eE]+)', text)]
    print('landscape loss per epoch:', losses)
    assert len(losses) == 2 and np.isfinite(losses).all(), text
    assert losses[1] < losses[0], losses
    assert os.path.exists(f'{run}/model_final_grasp_readout.pt') and os.path.exists(f'{run}/valid/results-2.pkl')
    sc, inputs, labels, model = case('v1b1p1_6d')
    model.compile(loss=lambda y, p: ((y - p) ** 2).mean(), learning_rate=LR, fused_step=True, fused_optimizer=True)
    with pytest.raises(ValueError, match='fused_step'):          # a custom loss is refused, as under --fused-step
        model.train_step((inputs, labels), sc['features'])
