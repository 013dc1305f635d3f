"""References of the backward of the biased 3x3 convolution (csrc/conv3x3_bwd.hip, ops.conv3x3_pack_transposed, encoders.Conv3x3BiasFunction;
DESIGN.md 18), shared by tests/test_conv3x3_bwd_cpu.py, tests/test_gpu_conv3x3_bwd.py and tests/test_gpu_fused_backward.py.  Written from the
definition and not by calling the package.  For y = conv3x3_same(act_in(x), W) + bias and g = dL/dy, NHWC maps, HWIO kernel:

    dw[dy,dx,ci,co] = sum_{n,i,j} act_in(x)[n,i+dy-1,j+dx-1,ci] g[n,i,j,co]          dbias[co] = sum_{n,i,j} g[n,i,j,co]
    dx[n,i,j,ci]    = act_in'(x)[n,i,j,ci] sum_{dy,dx,co} g[n,i-dy+1,j-dx+1,co] W[dy,dx,ci,co]         (taps outside the image 0)

* :func:`dw_ref`, :func:`dbias_ref`, :func:`dx_ref` - the definitions in float64.
* :func:`split_wgrad` - a NumPy restatement of the weight-gradient kernel's arithmetic: power-of-two scales from the two amax words, g cut
  like a weight and act_in(x) like an activation, three products, an fp32 sum per stage (half a 16 x 16 tile), fp32 slab sums in tile
  order, the slabs in double, one rounding.  :func:`split_dgrad` - the data gradient as the forward's restatement (conv3x3_ref.split_conv)
  on the flipped, transposed kernel, times act_in'.  `defect=` plants one wrong reading.
* :func:`e32` - the yardstick: float32 torch CPU autograd of the same case against the float64 references."""
import numpy as np

from tests import conv3x3_ref as R

TILE, STAGE_ROWS, SLAB_TILES = 16, 8, 16           # csrc/mvnerf_conv.h: kWgradTile, the stage of conv3x3_bwd.hip, kWgradSlabTiles
SLAB_PIXELS = SLAB_TILES * TILE * TILE
BAR = R.BAR
MIN_PIXELS = 30                                    # the accuracy bar is asserted on shapes with N h w >= 30; below, the exact tests
ACTS = [None, 'relu', 'elu']

# (N, h, w, Cin, Cout)
SMALL = (2, 3, 5, 32, 64)
TILED = (2, 19, 35, 64, 128)
WIDE_IN = (3, 33, 17, 128, 64)
DEEP = (1, 4, 4, 256, 64)
# from the slab constant: 3 x 3 x 5 = 45 tiles = 2 full slabs and a ragged third of 13 tiles, ragged tiles both ways
SLABS = (3, 2 * TILE + 1, 4 * TILE + 1, 32, 64)
assert 2 * SLAB_TILES < 3 * 3 * 5 < 3 * SLAB_TILES
GPU_SHAPES = [SMALL, TILED, WIDE_IN, DEEP, SLABS]


def inputs(shape, seed=0, scale_x=1.0, scale_g=1.0):
    """Seeded x (N,h,w,Cin), g (N,h,w,Cout) unit normals times the scales, a Glorot-uniform HWIO kernel and a bias; float32."""
    n, h, w, cin, cout = shape
    rng = np.random.default_rng([seed, 18, *shape])
    x = (rng.standard_normal((n, h, w, cin)) * scale_x).astype(np.float32)
    g = (rng.standard_normal((n, h, w, cout)) * scale_g).astype(np.float32)
    lim = np.sqrt(6.0 / (9 * cin + 9 * cout))
    wt = rng.uniform(-lim, lim, (3, 3, cin, cout)).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    return x, g, wt, bias


def act_grad(x, name):
    if name is None:
        return np.ones_like(x)
    if name == 'relu':
        return (x > 0).astype(x.dtype)
    if name == 'elu':
        return np.where(x > 0, 1.0, np.exp(np.minimum(x, 0))).astype(x.dtype)
    raise ValueError(name)


def _pad(x, mode='constant'):
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode=mode)


def dw_ref(x, g, act_in=None):
    xa = _pad(R.activation(np.asarray(x, np.float64), act_in))
    g = np.asarray(g, np.float64)
    n, h, w, cin = x.shape
    dw = np.zeros((3, 3, cin, g.shape[3]))
    for dy in range(3):
        for dx in range(3):
            dw[dy, dx] = np.einsum('nijc,nijo->co', xa[:, dy:dy + h, dx:dx + w], g)
    return dw


def dbias_ref(g):
    return np.asarray(g, np.float64).sum((0, 1, 2))


def flip_transpose(wt):
    """W'[dy,dx,co,ci] = W[2-dy,2-dx,ci,co]: the kernel whose forward convolution of g is the data gradient."""
    return np.ascontiguousarray(np.swapaxes(np.asarray(wt)[::-1, ::-1], 2, 3))


def dx_ref(x, g, wt, act_in=None):
    x = np.asarray(x, np.float64)
    gp = _pad(np.asarray(g, np.float64))
    wt = np.asarray(wt, np.float64)
    n, h, w, cin = x.shape
    dx = np.zeros_like(x)
    for dy in range(3):
        for ddx in range(3):
            # y[i] reads x[i + dy - 1], so x[i] is read by y[i - dy + 1]: the padded g at offset 2 - dy
            dx += gp[:, 2 - dy:2 - dy + h, 2 - ddx:2 - ddx + w] @ wt[dy, ddx].T
    return dx * act_grad(x, act_in)


def torch_grads(x, g, wt, bias, act_in, dtype):
    """torch CPU autograd of sum(g * (conv2d(pad(act_in(x))) + bias)) in `dtype` -> (dx NHWC, dw HWIO, dbias) arrays."""
    import torch
    import torch.nn.functional as F
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype)
    xt = t(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wo = t(wt).permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    bt = t(bias).requires_grad_(True)
    xa = {None: lambda v: v, 'relu': F.relu, 'elu': F.elu}[act_in](xt)
    y = F.conv2d(xa, wo, bt, padding=1)
    y.backward(t(g).permute(0, 3, 1, 2).contiguous())
    return (xt.grad.permute(0, 2, 3, 1).contiguous().numpy(), wo.grad.permute(2, 3, 1, 0).contiguous().numpy(), bt.grad.numpy())


_e32 = {}


def e32(shape, act_in, seed=0, scale_x=1.0, scale_g=1.0, mask_g=False):
    """{'dx' | 'dw' | 'dbias': (relative L2, worst element)} of the float32 torch CPU autograd run against the float64 references."""
    key = (tuple(shape), act_in, seed, scale_x, scale_g, mask_g)
    if key not in _e32:
        import torch
        x, g, wt, bias = case(shape, seed, scale_x, scale_g, mask_g)
        got = torch_grads(x, g, wt, bias, act_in, torch.float32)
        ref = (dx_ref(x, g, wt, act_in), dw_ref(x, g, act_in), dbias_ref(g))
        _e32[key] = {name: R.errors(a, b) for name, a, b in zip(('dx', 'dw', 'dbias'), got, ref)}
    return _e32[key]


def case(shape, seed=0, scale_x=1.0, scale_g=1.0, mask_g=False):
    x, g, wt, bias = inputs(shape, seed, scale_x, scale_g)
    if mask_g:                                     # half of g zeroed (a relu behind the convolution)
        g = g * (np.random.default_rng([seed, 19, *shape]).random(g.shape) < 0.5)
    return x, g.astype(np.float32), wt, bias


def within_bar(got, ref, yard, bar=BAR):
    """[(ratio of relative L2, ratio of worst element)] <= bar, both."""
    err = R.errors(got, ref)
    return all(e <= bar * y for e, y in zip(err, yard)), tuple(e / y if y else float('inf') if e else 0.0 for e, y in zip(err, yard))


# ---- the kernels' arithmetic --------------------------------------------------------------------------------------------------------------
def tiles_of(n, h, w):
    """The kernel's tile order: [image][tile row][tile column] -> (image, y0, x0)."""
    return [(i, y0, x0) for i in range(n) for y0 in range(0, h, TILE) for x0 in range(0, w, TILE)]


WGRAD_DEFECTS = ['shift_reversed', 'clamp_padding', 'ragged_counted', 'batch_leak', 'act_missing', 'dbias_wrong_axis', 'drop_a1_b0',
                 'drop_a0s_b1', 'scale_kept', 'last_slab_skipped']
DGRAD_DEFECTS = ['taps_not_flipped', 'taps_transposed', 'act_grad_missing', 'elu_grad_one']


def split_wgrad(x, g, act_in=None, amax_x=None, amax_g=None, defect=None):
    """The weight-gradient kernel's arithmetic in NumPy -> (dw (3,3,Cin,Cout), dbias (Cout,)) float32.  The three products of a stage are
    summed in float64 (exact for fp16 factors) and rounded into fp32; the MFMA rounds per k-step and truncates, so the kernel sits a
    little above this."""
    x, g = np.asarray(x, np.float32), np.asarray(g, np.float32)
    n, h, w, cin = x.shape
    cout = g.shape[3]
    amax_x = np.float32(np.abs(x).max() if amax_x is None else amax_x)
    amax_g = np.float32(np.abs(g).max() if amax_g is None else amax_g)
    if not (np.isfinite(amax_x) and np.isfinite(amax_g)):
        return np.full((3, 3, cin, cout), np.nan, np.float32), np.full(cout, np.nan, np.float32)
    if defect == 'dbias_wrong_axis':
        dbias = g.reshape(-1).reshape(cout, -1).astype(np.float64).sum(1)
    else:
        dbias = g.astype(np.float64).sum((0, 1, 2))
    dbias = (np.zeros(cout) if amax_g == 0 else dbias).astype(np.float32)
    if amax_x == 0 or amax_g == 0:
        return np.zeros((3, 3, cin, cout), np.float32), dbias
    ex, eg = R.scale_exp(amax_x), R.scale_exp(amax_g)
    xa = x if defect == 'act_missing' else R.activation(x, act_in).astype(np.float32)
    if defect == 'batch_leak':                     # the images as one tall map: rows of the neighbour behind the top and bottom edges
        xa, g, n, h = xa.reshape(1, n * h, w, cin), g.reshape(1, n * h, w, cout), 1, n * h
    th, tw = -(-h // TILE) * TILE, -(-w // TILE) * TILE
    room = ((0, 0), (1, th - h + 1), (1, tw - w + 1), (0, 0))
    b0, b1 = (np.pad(p.astype(np.float64), room, mode='edge' if defect == 'clamp_padding' else 'constant') for p in R.cut_act(xa, ex))
    groom = ((0, 0), (0, th - h), (0, tw - w), (0, 0))
    a0, a1, a0s = (np.pad(p.astype(np.float64), groom, mode='edge' if defect == 'ragged_counted' else 'constant') for p in R.cut_weight(g, eg))
    tiles = tiles_of(n, h, w)
    total = np.zeros((3, 3, cin, cout))
    slabs = [tiles[i:i + SLAB_TILES] for i in range(0, len(tiles), SLAB_TILES)]
    if defect == 'last_slab_skipped' and len(slabs) > 1 and len(slabs[-1]) < SLAB_TILES:
        slabs = slabs[:-1]
    for slab in slabs:
        part = np.zeros((3, 3, cin, cout), np.float32)
        for i, y0, x0 in slab:
            for yh in (y0, y0 + STAGE_ROWS):
                if yh >= h:
                    break
                gs = [p[i, yh:yh + STAGE_ROWS, x0:x0 + TILE].reshape(-1, cout) for p in (a0, a1, a0s)]
                stage = np.zeros((3, 3, cin, cout))
                for dy in range(3):
                    for dx in range(3):
                        oy, ox = (2 - dy, 2 - dx) if defect == 'shift_reversed' else (dy, dx)
                        x0s, x1s = (p[i, yh + oy:yh + oy + STAGE_ROWS, x0 + ox:x0 + ox + TILE].reshape(-1, cin) for p in (b0, b1))
                        s = x0s.T @ gs[0]
                        if defect != 'drop_a0s_b1':
                            s = s + x1s.T @ gs[2]
                        if defect != 'drop_a1_b0':
                            s = s + x0s.T @ gs[1]
                        stage[dy, dx] = s
                part = (part.astype(np.float64) + stage.astype(np.float32)).astype(np.float32)
        total += part
    undo = -(ex + (0 if defect == 'scale_kept' else eg))
    with np.errstate(over='ignore'):
        return np.ldexp(total, undo).astype(np.float32), dbias


def split_dgrad(x, g, wt, act_in=None, amax_g=None, defect=None):
    """The data gradient's arithmetic: the forward's restatement on g with the flipped, transposed kernel, times act_in'(x) in float32."""
    wt = np.asarray(wt, np.float32)
    back = flip_transpose(wt)
    if defect == 'taps_not_flipped':
        back = np.ascontiguousarray(np.swapaxes(wt, 2, 3))
    if defect == 'taps_transposed':
        back = np.ascontiguousarray(np.swapaxes(back, 0, 1))
    dx = R.split_conv(np.asarray(g, np.float32), None, back, amax_a=amax_g)
    x = np.asarray(x, np.float32)
    if defect == 'act_grad_missing':
        return dx
    if defect == 'elu_grad_one' and act_in == 'elu':
        return dx
    return (dx * act_grad(x, act_in)).astype(np.float32)
