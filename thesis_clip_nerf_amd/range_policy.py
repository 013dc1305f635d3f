"""What to do when a net or a frame leaves the range of the fp16 two-piece field kernel (f32_gemm='split_f16').

The kernel's weight pieces are rn16(64 w) and its activation pieces rn16(v / 64); fp16 rounds to infinity from 65520 upward, so it
is correct for |w| < 1023.75 and |v| < 4193280 and silently wrong beyond.  The training backward cuts relu(stashed pre-activation) as
rn16(64 a): for a training step every pre-activation has to stay below the WEIGHT limit.  The measured maxima come from
ops.net_range (weights) and from the range status of the guarded kernel (activations); this module only decides.  It is a pure
function of its arguments - no device, no library - so that the whole truth table can be tested anywhere."""
from __future__ import annotations

import math

from ._lib import F16X3_MAX_ACT, F16X3_MAX_WEIGHT

POLICIES = ('fallback', 'raise', 'off')
RUN, FALLBACK, RAISE = 'run', 'fallback', 'raise'


def limits(training=False):
    """(weight limit, activation limit): inference, or - training=True - a training step (the backward's limit on pre-activations)."""
    return F16X3_MAX_WEIGHT, (F16X3_MAX_WEIGHT if training else F16X3_MAX_ACT)


def below(value, limit):
    """value < limit, with None (not measured) in range and NaN / infinity out of it."""
    return value is None or (not math.isnan(value) and value < limit)


def worst(values):
    """The largest of the measured maxima, a NaN counting as larger than everything."""
    return max(values, key=lambda x: math.inf if math.isnan(x) else x)


def in_range(max_weight, max_activation, training=False):
    w_lim, a_lim = limits(training)
    return below(max_weight, w_lim) and below(max_activation, a_lim)


def decide(policy, kernel, max_weight=None, max_activation=None, training=False):
    """-> RUN (stay on `kernel`), FALLBACK (run 'split_bf16' instead, with a warning) or RAISE (FloatingPointError).
    Only 'split_f16' has a range; policy 'off' never looks.  A training step cannot fall back (its backward has one form): out of
    range it raises under 'fallback' as well."""
    if policy not in POLICIES:
        raise ValueError(f'range_policy must be one of {POLICIES}, got {policy!r}')
    if policy == 'off' or kernel != 'split_f16' or in_range(max_weight, max_activation, training):
        return RUN
    return RAISE if policy == 'raise' or training else FALLBACK


def describe(max_weight, max_activation, training=False):
    """The message of the warning / error: which maximum passed which limit."""
    w_lim, a_lim = limits(training)
    parts = []
    if not below(max_weight, w_lim):
        parts.append(f'max |weight| = {max_weight:g} is not below {w_lim:g}')
    if not below(max_activation, a_lim):
        what = 'max pre-activation (the backward cuts it as rn16(64 a))' if training else 'max |activation|'
        parts.append(f'{what} = {max_activation:g} is not below {a_lim:g}')
    return "outside the range of f32_gemm='split_f16': " + '; '.join(parts)
