"""dcs_level_gain (host only) against the numpy float32 restatement (tests/level_ref.py), bit for bit: the gain and the
resulting peak for every mode over the whole positive float32 range, around each ceiling, and at the range's ends; the
fitted peak never above the ceiling; every invalid argument refused."""
import ctypes

import numpy as np
import pytest

import level_ref as LR
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_INVALID_ARG, LEVEL_CLIP, LEVEL_FIT, LEVEL_GAIN, LEVEL_NORMALIZE, DcsError, Level

F32 = np.float32
CEILINGS = [F32(1.0), F32(0.8912509), F32(0.5)]
TINY, FLT_MAX = np.finfo(F32).smallest_subnormal, np.finfo(F32).max
INF = float("inf")


def bits(x):
    return int(np.asarray(x, F32).view(np.uint32))


def peaks():
    """seeded bit patterns over every positive finite float32 (subnormals included), 1 to 50 ulps above each ceiling and a
    few below, the ceilings themselves, and the ends of the range"""
    rng = np.random.default_rng(0x1E7E1)
    out = list(rng.integers(1, 0x7F800000, 3000).astype(np.uint32).view(F32))
    out += list(rng.integers(1, 0x00800000, 300).astype(np.uint32).view(F32))           # subnormals
    for c in CEILINGS:
        b = bits(c)
        out += list(np.arange(b - 5, b + 51, dtype=np.uint32).view(F32))
    out += [F32(0), TINY, np.finfo(F32).tiny, FLT_MAX, np.nextafter(FLT_MAX, F32(0)), F32(1.21), F32(1.044)]
    return out


def call(dcs, peak, mode, flags=0, gain=1.0, ceiling=1.0, bound=INF):
    """-> (status, gain, peak_out) of dcs_level_gain"""
    g, p = ctypes.c_float(-7), ctypes.c_float(-7)
    st = dcs.load_library().dcs_level_gain(float(peak), ctypes.byref(Level(mode, flags, gain, ceiling)), float(bound), ctypes.byref(g),
                                           ctypes.byref(p))
    return st, F32(g.value), F32(p.value)


def test_fit_and_normalize_equal_the_restatement(dcs):
    steps = []
    for c in CEILINGS:
        for P in peaks():
            for mode in (LEVEL_FIT, LEVEL_NORMALIZE):
                for flags in (0, LEVEL_CLIP):
                    st, g, after = call(dcs, P, mode, flags, ceiling=c)
                    want_g, want_after = LR.gain(P, LR.Level(mode, flags, 1.0, c))
                    assert st == 0 and bits(g) == bits(want_g) and bits(after) == bits(want_after), (P, c, mode, flags)
                    assert after == F32(P * g) and (after <= c or (mode == LEVEL_FIT and P <= c))
                    if mode == LEVEL_FIT and P <= c:
                        assert g == 1 and after == P
                    if mode == LEVEL_NORMALIZE and P == 0:
                        assert g == 1 and after == 0
            if P > 0:
                LR.fit_gain(P, c, steps)
    # the rule is written as a loop; these peaks never need more than one step of it
    assert max(steps) <= 1 and 1 in steps


def test_normalize_reaches_the_ceiling_from_either_side(dcs):
    for c in CEILINGS:
        for P in (TINY, F32(1e-30), F32(0.25), c, np.nextafter(c, F32(2)), F32(3.0), FLT_MAX):
            st, g, after = call(dcs, P, LEVEL_NORMALIZE, ceiling=c)
            assert st == 0 and after <= c
            # c / P rounds by half an ulp, the loop steps down at most one more, the product rounds by half an ulp again:
            # the peak lands within four parts in 2^23 of the ceiling (unless no float32 gain is large enough)
            assert g == FLT_MAX or float(after) >= float(c) * (1 - 4 * 2.0 ** -23)


def test_gain_equals_the_restatement(dcs):
    rng = np.random.default_rng(0x6A14)
    gains = [F32(1), F32(0.5), F32(2), TINY, FLT_MAX, F32(1e-20), F32(0.8264462)] + list(rng.integers(1, 0x7F800000, 40).astype(np.uint32).view(F32))
    for P in peaks()[::7] + [F32(0), TINY, FLT_MAX]:
        for gain in gains:
            for flags in (0, LEVEL_CLIP):
                st, g, after = call(dcs, P, LEVEL_GAIN, flags, gain=gain, ceiling=0.5)
                want_g, want_after = LR.gain(P, LR.Level(LEVEL_GAIN, flags, gain, 0.5))
                assert bits(g) == bits(gain) == bits(want_g) and bits(after) == bits(want_after), (P, gain, flags)
                assert st == 0                  # (bound infinite: an overflowing product is reported, not refused)
                if flags:
                    assert after <= F32(0.5)


def test_bound(dcs):
    """the peak that comes out is compared with the caller's bound: above it is DCS_ERR_BAD_STREAM with both values filled"""
    assert call(dcs, 0.9, LEVEL_GAIN, gain=1.0, bound=1.0)[0] == 0
    st, g, after = call(dcs, 0.9, LEVEL_GAIN, gain=1.5, bound=1.0)
    assert st == ERR_BAD_STREAM and g == F32(1.5) and after == F32(F32(0.9) * F32(1.5))
    assert call(dcs, 0.9, LEVEL_GAIN, LEVEL_CLIP, gain=1.5, ceiling=1.0, bound=1.0) == (0, F32(1.5), F32(1.0))
    b16 = F32(32768) / F32(32767)
    assert call(dcs, b16, LEVEL_GAIN, gain=1.0, bound=b16)[0] == 0
    assert call(dcs, np.nextafter(b16, F32(2)), LEVEL_GAIN, gain=1.0, bound=b16)[0] == ERR_BAD_STREAM
    assert call(dcs, 1.21, LEVEL_FIT, bound=1.0) == (0,) + LR.gain(1.21, LR.Level(LEVEL_FIT))
    assert call(dcs, FLT_MAX, LEVEL_GAIN, gain=2.0, bound=FLT_MAX)[0] == ERR_BAD_STREAM      # overflows to infinity
    from dcsexplorer_amd import level_gain
    assert level_gain(1.21, Level(LEVEL_FIT)) == LR.gain(1.21, LR.Level(LEVEL_FIT))
    with pytest.raises(DcsError) as e:
        level_gain(0.9, Level(LEVEL_GAIN, gain=1.5))
    assert e.value.status == ERR_BAD_STREAM and e.value.peak_out == F32(F32(0.9) * F32(1.5))


@pytest.mark.parametrize("what,kw", [
    ("mode 0", dict(mode=0)), ("mode 4", dict(mode=4)), ("mode 0xFFFFFFFF", dict(mode=0xFFFFFFFF)),
    ("flag 2", dict(flags=2)), ("flag 0x80000000", dict(flags=0x80000000)), ("flags 3", dict(flags=3)),
    ("gain 0", dict(mode=LEVEL_GAIN, gain=0.0)), ("gain -0.0", dict(mode=LEVEL_GAIN, gain=-0.0)),
    ("gain negative", dict(mode=LEVEL_GAIN, gain=-1.0)), ("gain inf", dict(mode=LEVEL_GAIN, gain=INF)),
    ("gain nan", dict(mode=LEVEL_GAIN, gain=float("nan"))),
    ("ceiling 0", dict(ceiling=0.0)), ("ceiling negative", dict(ceiling=-0.5)), ("ceiling above 1", dict(ceiling=1.0000001)),
    ("ceiling inf", dict(ceiling=INF)), ("ceiling nan", dict(ceiling=float("nan"))),
    ("ceiling 0 with GAIN", dict(mode=LEVEL_GAIN, ceiling=0.0)), ("ceiling 2 with NORMALIZE", dict(mode=LEVEL_NORMALIZE, ceiling=2.0)),
    ("peak negative", dict(peak=-0.5)), ("peak inf", dict(peak=INF)), ("peak nan", dict(peak=float("nan"))),
    ("bound 0", dict(bound=0.0)), ("bound negative", dict(bound=-1.0)), ("bound nan", dict(bound=float("nan")))])
def test_invalid_arguments(dcs, what, kw):
    a = dict(peak=0.5, mode=LEVEL_FIT, flags=0, gain=1.0, ceiling=1.0, bound=1.0)
    a.update(kw)
    st, g, after = call(dcs, **a)
    assert st == ERR_INVALID_ARG and g == -7 and after == -7, what
    if "peak" not in kw and "bound" not in kw:
        assert not LR.valid(LR.Level(a["mode"], a["flags"], a["gain"], a["ceiling"])), what


def test_null_pointers_and_valid_edges(dcs):
    L = dcs.load_library()
    g, p = ctypes.c_float(), ctypes.c_float()
    lv = Level(LEVEL_FIT)
    assert L.dcs_level_gain(0.5, None, 1.0, ctypes.byref(g), ctypes.byref(p)) == ERR_INVALID_ARG
    assert L.dcs_level_gain(0.5, ctypes.byref(lv), 1.0, None, ctypes.byref(p)) == ERR_INVALID_ARG
    assert L.dcs_level_gain(0.5, ctypes.byref(lv), 1.0, ctypes.byref(g), None) == ERR_INVALID_ARG
    # what is just inside: the smallest ceiling and gain, ceiling 1, a gain the other modes do not read, peak -0.0
    assert call(dcs, 0.5, LEVEL_FIT, ceiling=TINY)[0] == 0
    assert call(dcs, 0.5, LEVEL_GAIN, gain=TINY, ceiling=1.0)[0] == 0
    assert call(dcs, 0.5, LEVEL_FIT, gain=float("nan"))[0] == 0 and call(dcs, 0.5, LEVEL_NORMALIZE, gain=-1.0)[0] == 0
    assert call(dcs, -0.0, LEVEL_NORMALIZE)[:2] == (0, F32(1))
    assert LR.valid(LR.Level(LEVEL_FIT, 0, float("nan"), TINY))


def test_struct_sizes(dcs):
    assert ctypes.sizeof(Level) == 16 and dcs.LEVEL_INFO_DTYPE.itemsize == 24
    assert [dcs.LEVEL_INFO_DTYPE.fields[k][1] for k in ("peakIn", "gain", "peakOut", "mode", "nClipped")] == [0, 4, 8, 12, 16]
