"""A numpy float32 restatement of the library's level stage (dcs_level_gain, dcs_level_streams and the level argument of
the resampling and encoding entry points; INTEGRATION.md "Level").

Every step is one float32 operation with one rounding, as the library's: the division of fit_gain, the product P * g that
is compared with the ceiling, and the product y * g per sample.  numpy keeps float32 subnormals and does not contract."""
import collections

import numpy as np

F32 = np.float32
GAIN, FIT, NORMALIZE = 1, 2, 3
CLIP = 1
FLT_MAX = np.finfo(F32).max

Level = collections.namedtuple("Level", "mode flags gain ceiling", defaults=(0, 1.0, 1.0))
Refused = collections.namedtuple("Refused", "status peak_in gain peak_out")
INVALID_ARG, BAD_STREAM = -1, -6


def valid(level):
    if level.mode not in (GAIN, FIT, NORMALIZE) or level.flags & ~CLIP:
        return False
    g, c = F32(level.gain), F32(level.ceiling)
    if level.mode == GAIN and not (np.isfinite(g) and g > 0):
        return False
    return bool(c > 0 and c <= 1)


def fit_gain(peak, ceiling, steps=None):
    """the correctly rounded c / P, stepped towards 0 while float32(P * g) > c; steps (a list) takes the number of nextafter
    steps the loop made"""
    P, c = F32(peak), F32(ceiling)
    with np.errstate(over="ignore", divide="ignore"):
        g = F32(c / P)
    if np.isinf(g):
        g = FLT_MAX
    n = 0
    while F32(P * g) > c:
        g = np.nextafter(g, F32(0))
        n += 1
    if steps is not None:
        steps.append(n)
    return g


def gain(peak, level):
    """-> (g, peak_out) as float32 for a finite peak >= 0 and a valid level"""
    P, c = F32(peak), F32(level.ceiling)
    g = F32(1)
    if level.mode == GAIN:
        g = F32(level.gain)
    elif (P > c) if level.mode == FIT else (P != 0):
        g = fit_gain(P, c)
    with np.errstate(over="ignore"):
        after = F32(P * g)
    if level.flags & CLIP and after > c:
        after = c
    return g, after


def apply(y, level, bound=1.0):
    """-> (y', peak_in, gain, peak_out, n_clipped), or Refused: INVALID_ARG for a bad level, BAD_STREAM for a sample that is
    not finite or a peak that comes out above bound"""
    y = np.asarray(y, dtype=F32)
    if not valid(level):
        return Refused(INVALID_ARG, None, None, None)
    if not np.isfinite(y).all():
        return Refused(BAD_STREAM, None, None, None)
    P = np.abs(y).max() if len(y) else F32(0)
    g, after = gain(P, level)
    if not after <= F32(bound):
        return Refused(BAD_STREAM, P, g, after)
    c = F32(level.ceiling)
    with np.errstate(over="ignore", under="ignore"):
        out = (y * g).astype(F32)           # (g == 1 leaves every bit as it is, -0.0 and subnormals included)
    n_clipped = 0
    if level.flags & CLIP:                  # (FIT and NORMALIZE end at or below the ceiling: the clamp finds nothing)
        over = np.abs(out) > c
        n_clipped = int(over.sum())
        out = np.where(over, np.copysign(c, out), out).astype(F32)
    return out, P, g, after, n_clipped
