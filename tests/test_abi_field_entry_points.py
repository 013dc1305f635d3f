"""Argument validation of the field-pass, texel-table and render entry points of the C ABI, one fault at a time.

Every entry point gets a valid baseline argument list built from fake device pointers (as tests/test_abi.py does) and then
one row per fault: a required pointer NULL, a pointer that must be 16-byte aligned moved off its alignment, a size set to 0,
H or W set to 1, and the entry point's own limits.  Each row asserts the return code and that the message names the entry
point's family.  Validation returns before anything is launched, so no GPU is needed - and, because the pointers are fake,
only faults that are caught before the first launch may appear here (see RENDER below).

The expected codes were recorded by running this table against the library as it was BEFORE the validation was
consolidated into one routine; they pin that behaviour, inconsistencies included (H < 2 is a shape error from five field
entry points and an argument error from the stash pair and from project_texels*).  The one row that was added with the
consolidation is marked `differs_from_parent`.
"""
import ctypes

import pytest

from thesis_clip_nerf_amd import _lib

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -3

# everything that is not a pointer, by argument name
BASE = {'B': 1, 'V': 1, 'R': 4, 'S': 64, 'N': 40, 'H': 8, 'W': 8, 'near_': 0.3, 'far_': 1.3, 'q7_mode': 0, 'tables_ready': 0}

# Argument lists in ABI order (include/mvnerf_hip.h).  name* = must be 16-byte aligned, name? = optional (NULL in the baseline),
# name~ = required, but only checked after the entry point's first launch: never faulted here.
_FIELD_IN = 'rays_o rays_d z images features* '
_FIELD_CAM = 'intrinsics extrinsics_inv packed_net* '
_DIMS = 'B V R S H W '
_FIELD_OUT = 'rgbs* tap_idx?* pix? embedding?* acts_per_view?* acts_fused?* workspace* stream?'
_BF16_OUT = 'rgbs* tap_idx?* embedding?* acts_fused?* workspace* stream?'
_STASH_OUT = 'rgbs* stash* workspace* stream?'
_TEXELS = ' B V H W texel_table* texel_table_b? stream?'
_RENDER_IN = 'rays_o~ rays_d~ images~ features~ intrinsics~ extrinsics_inv~ packed_coarse~ packed_fine '
_RENDER_OUT = ('u_coarse u_fine B V R S H W near_ far_ q7_mode rgb depth fine_rgb fine_depth workspace* texel_tables? '
               'tables_ready stream?')
# the backward and query entry points (recorded before their stash arithmetic and their walk through the trunk were shared)
_BACKWARD = ('rays_o rays_d z images features texel_table?* texel_grad?* intrinsics extrinsics_inv net_keras* bwd_streams* stash* rgbs* '
             'd_rgbs* B V R S H W scratch* grad d_z? d_features? stream?')
_QUERY_VJP = ('points dirs images features* intrinsics extrinsics_inv bwd_streams* stash* g_acts* B V N H W scratch* d_points d_dirs '
              'stream?')
_QUERY_JVP = ('points dirs t_points t_dirs images features* intrinsics extrinsics_inv packed_net* B V N H W acts?* t_acts* workspace* '
              'stream?')

FIELD_CODES = {'null': E_ARG, 'misaligned': E_ALIGN, 'zero': E_ARG, 'hw1': E_SHAPE}
STASH_CODES = {'null': E_ARG, 'misaligned': E_ALIGN, 'zero': E_ARG, 'hw1': E_ARG}
TEXEL_CODES = {'null': E_ARG, 'misaligned': E_ALIGN, 'zero': E_ARG, 'hw1': E_ARG}
RENDER_CODES = {'null': E_ARG, 'misaligned': E_ALIGN, 'zero': E_ARG}

TOO_MANY_SAMPLES = dict(B=32768, R=65536, S=1)            # B*R*S = 2^31
TOO_MANY_TEXELS = dict(H=65536, W=32768)                  # B*V*H*W = 2^31
# (label, overrides, code, message substring, differs_from_parent)
INT32_ROWS = [('B*R*S=2^31', TOO_MANY_SAMPLES, E_SHAPE, '', False), ('B*V*H*W=2^31', TOO_MANY_TEXELS, E_SHAPE, '', False)]
STASH_ROWS = [('V=2,R*S=15', dict(V=2, R=15, S=1), E_SHAPE, 'multiple of 32', False),
              ('262143-tile limit', dict(B=8, V=3, R=16384, S=128), E_SHAPE, 'at most 262143', False),
              ('B*R*S=2^31', TOO_MANY_SAMPLES, E_SHAPE, '', False),
              # the stash pair launches the same kernels with the same int32 texel indices as the other five and gained their check
              ('B*V*H*W=2^31', TOO_MANY_TEXELS, E_SHAPE, '', True)]
# the second net and the second table go together; given together, both are checked for alignment
TEXEL_ROWS = [('second net without its table', dict(second_net=0), E_ARG, 'go together', False),
              ('second table without its net', dict(texel_table_b=0), E_ARG, 'go together', False),
              ('misaligned second net', dict(second_net=4, texel_table_b=0), E_ALIGN, '', False),
              ('misaligned second table', dict(second_net=0, texel_table_b=4), E_ALIGN, '', False),
              ('B*V*H*W=2^31', TOO_MANY_TEXELS, E_SHAPE, '', False)]
# mvnerf_render_fwd* check V, H, W and the scene pointers in their field passes, after the depth launch: with fake pointers only
# what the entry point itself checks up front can be faulted (S first, so S = 0 is a shape error like every S != 64)
RENDER_ROWS = [('S=32', dict(S=32), E_SHAPE, 'n_samples=64', False), ('S=128', dict(S=128), E_SHAPE, 'n_samples=64', False),
               ('S=0', dict(S=0), E_SHAPE, 'n_samples=64', False)]
BACKWARD_CODES = {'null': E_ARG, 'misaligned': E_ALIGN, 'zero': E_ARG, 'hw1': E_ARG}
QUERY_JVP_CODES = {'null': E_ARG, 'misaligned': E_ALIGN, 'zero': E_ARG, 'hw1': E_SHAPE}
FUSED_ACTS_CODES = {'null': E_ARG, 'misaligned': E_ALIGN, 'zero': E_ARG}
# V = 2 with a row count that is no multiple of 32: refused where the per-view tiles are walked; the tangent pass and the fused
# activations have no such limit and go on to launch (code None: as the baseline)
BACKWARD_ROWS = [('V=2,R*S=15', dict(V=2, R=15, S=1), E_SHAPE, 'multiple of 32', False)]
QUERY_VJP_ROWS = [('V=2,N=40', dict(V=2), E_SHAPE, 'multiple of 32', False)]
NO_TILE_LIMIT_ROWS = [('V=2,N=40 passes', dict(V=2), None, '', False)]

# name, family the message must name, arguments, sizes that may not be 0, codes per fault class, extra rows
ENTRY_POINTS = [
    ('mvnerf_field_eval', 'mvnerf_field_eval', _FIELD_IN + _FIELD_CAM + _DIMS + _FIELD_OUT, 'BVRS', FIELD_CODES, INT32_ROWS),
    ('mvnerf_field_eval_table', 'mvnerf_field_eval', _FIELD_IN + 'texel_table* ' + _FIELD_CAM + _DIMS + _FIELD_OUT, 'BVRS', FIELD_CODES,
     INT32_ROWS),
    ('mvnerf_field_eval_bf16', 'mvnerf_field_eval_bf16', _FIELD_IN + 'texel_table?* ' + _FIELD_CAM + 'packed16* ' + _DIMS + _BF16_OUT,
     'BVRS', FIELD_CODES, INT32_ROWS),
    ('mvnerf_field_eval_bf16maps', 'mvnerf_field_eval_bf16maps',
     _FIELD_IN + 'texel_table?* ' + _FIELD_CAM + 'packed16* ' + _DIMS + _BF16_OUT, 'BVRS', FIELD_CODES, INT32_ROWS),
    ('mvnerf_field_eval_split', 'mvnerf_field_eval_split',
     _FIELD_IN + 'texel_table?* ' + _FIELD_CAM + 'packed_split* ' + _DIMS + _FIELD_OUT, 'BVRS', FIELD_CODES, INT32_ROWS),
    ('mvnerf_field_eval_stash', 'mvnerf_field_eval_stash', _FIELD_IN + 'texel_table?* ' + _FIELD_CAM + _DIMS + _STASH_OUT, 'BVRS',
     STASH_CODES, STASH_ROWS),
    ('mvnerf_field_eval_stash_split', 'mvnerf_field_eval_stash_split',
     _FIELD_IN + 'texel_table?* ' + _FIELD_CAM + 'packed_split* ' + _DIMS + _STASH_OUT, 'BVRS', STASH_CODES, STASH_ROWS),
    ('mvnerf_project_texels2', 'mvnerf_project_texels', 'features* packed_net* second_net?' + _TEXELS, 'BV', TEXEL_CODES, TEXEL_ROWS),
    ('mvnerf_project_texels_bf16', 'mvnerf_project_texels_bf16', 'features* packed16* second_net?' + _TEXELS, 'BV', TEXEL_CODES, TEXEL_ROWS),
    ('mvnerf_project_texels_bf16maps', 'mvnerf_project_texels_bf16maps', 'features_bf16* packed16* second_net?' + _TEXELS, 'BV', TEXEL_CODES,
     TEXEL_ROWS),
    ('mvnerf_render_fwd', 'mvnerf_render_fwd', _RENDER_IN + _RENDER_OUT, 'BR', RENDER_CODES, RENDER_ROWS),
    ('mvnerf_render_fwd_split', 'mvnerf_render_fwd_split', _RENDER_IN + 'split_coarse split_fine ' + _RENDER_OUT, 'BR', RENDER_CODES,
     RENDER_ROWS),
    ('mvnerf_field_backward_table', 'mvnerf_field_backward', _BACKWARD, 'BVRS', BACKWARD_CODES, BACKWARD_ROWS),
    ('mvnerf_query_vjp', 'mvnerf_query_vjp', _QUERY_VJP, 'BVN', BACKWARD_CODES, QUERY_VJP_ROWS),
    ('mvnerf_query_jvp', 'mvnerf_query_jvp', _QUERY_JVP, 'BVN', QUERY_JVP_CODES, NO_TILE_LIMIT_ROWS),
    ('mvnerf_stash_fused_acts', 'mvnerf_stash_fused_acts', 'stash* B V N acts* stream?', 'BVN', FUSED_ACTS_CODES, NO_TILE_LIMIT_ROWS),
]


def _parse(spec):
    """-> [(name, is_pointer, required, aligned, faultable)] in ABI order."""
    args = []
    for tok in spec.split():
        name = tok.rstrip('*?~')
        args.append((name, name not in BASE, '?' not in tok, '*' in tok, '~' not in tok))
    return args


def _rows():
    for fn, family, spec, nonzero, codes, extra in ENTRY_POINTS:
        args = _parse(spec)
        yield fn, family, args, 'baseline', {}, None, '', False
        for name, is_ptr, required, aligned, faultable in args:
            if is_ptr and required and faultable:
                yield fn, family, args, f'null {name}', {name: None}, codes['null'], 'null', False
            if is_ptr and aligned:
                yield fn, family, args, f'misaligned {name}', {name: 4}, codes['misaligned'], 'aligned', False
        for d in nonzero:
            yield fn, family, args, f'{d}=0', {d: 0}, codes['zero'], '', False
        if 'hw1' in codes:
            for d in 'HW':
                yield fn, family, args, f'{d}=1', {d: 1}, codes['hw1'], '', False
        for label, over, code, text, differs in extra:
            yield fn, family, args, label, over, code, text, differs


def _call(fn, args, over):
    """Baseline: every required pointer a distinct fake 16-byte-aligned address, every optional one NULL.  An override of a
    pointer is None (NULL) or a byte offset from the argument's baseline address; of a size, the value."""
    values = []
    for i, (name, is_ptr, required, _, _) in enumerate(args):
        if not is_ptr:
            values.append(over.get(name, BASE[name]))
        elif name in over:
            values.append(None if over[name] is None else ctypes.c_void_p(4096 + 256 * i + over[name]))
        else:
            values.append(ctypes.c_void_p(4096 + 256 * i) if required else None)
    lib = _lib.lib()
    rc = getattr(lib, fn)(*values)
    return rc, lib.mvnerf_last_error().decode()


ROWS = list(_rows())


@pytest.mark.parametrize('fn,family,args,label,over,code,text,differs_from_parent', ROWS,
                         ids=[f'{r[0]}-{r[3]}' + ('-differs_from_parent' if r[7] else '') for r in ROWS])
def test_one_fault_at_a_time(fn, family, args, label, over, code, text, differs_from_parent):
    assert len(args) == len(_lib.SIGNATURES[fn][1])
    if code is None:
        # The baseline passes validation and goes on to launch: with fake pointers that may only happen where there is no GPU to
        # fault, and there the launch itself fails with a HIP error (> 0), which shows that no check objected.
        import torch
        if not torch.cuda.is_available():
            rc, msg = _call(fn, args, over)
            assert rc > 0, (rc, msg)
        return
    rc, msg = _call(fn, args, over)
    print(f'{fn} [{label}] -> {rc}: {msg}')
    assert rc == code, msg
    assert family in msg, msg
    assert text in msg, msg
