"""The level stage on the MI355X (dcs_level_streams, and the level argument of resample_streams, encode_streams_at and
encode_files) against its numpy float32 restatement (tests/level_ref.py), bit for bit: outputs, peaks, gains and clip counts.

The shapes are the smallest at which the scaling kernel can go wrong: streams of 0, 1, 3, 239, 240, 241 and 4 097 samples in
one call, so that every stream starts at another offset from a 16-byte boundary and has another head and tail around its
vector body, and one call of 65 537 streams of one to three samples, more than a grid's y dimension holds.

After the converter the expected floats are level_ref.apply(resample_ref.resample(...)).  On the default table
resample_ref gives the 44 100 Hz stereo square a peak of 1.2161008, the 48 000 Hz square 1.2098658 and the 31 250 Hz square
through the converter 1.0872074 (FIT scales them); the 8 000 Hz noise stays at 0.58210206 and the 31 250 Hz pass-through at
0.95 (FIT leaves them alone).  The float entry points refuse only a levelled peak that is not finite; the encoders keep
their bound of 1, or the source format's own full scale for a file.

The FLAC twin of fullscale_s16_31250 is 240 samples of -32768, 32767, -32768, 0: through the converter at 31 250 Hz its
peak is 0.7962882, so that call is accepted today and FIT leaves it alone; passed through (the default) it is 1.0000305,
inside the format's full scale but above a ceiling of 1, and FIT scales it.  Both are checked."""
import ctypes

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc93_ref as E93
import enc_ref as E
import flac_cases as FC
import flac_ref as FR
import level_ref as LR
import resample_ref as RS
import rs_cases
import wav_cases as WC
import wav_ref as WR
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_INVALID_ARG, LEVEL_CLIP, LEVEL_FIT, LEVEL_GAIN, LEVEL_NORMALIZE, DcsError, Level, _ptr

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
TINY = float(np.finfo(F32).smallest_subnormal)
LENGTHS = [0, 1, 3, 239, 240, 241, 4097]
same_bits = rs_cases.same_bits


def lv(level):
    """the library's Level of a level_ref.Level"""
    return Level(level.mode, level.flags, level.gain, level.ceiling)


def check_info(info, want, what):
    """a LEVEL_INFO_DTYPE record against level_ref.apply's (y', peak_in, gain, peak_out, n_clipped)"""
    _, p_in, g, p_out, n_clipped = want
    for got, exp in ((info["peakIn"], p_in), (info["gain"], g), (info["peakOut"], p_out)):
        assert F32(got).view(np.uint32) == F32(exp).view(np.uint32), (what, info, want[1:])
    assert info["nClipped"] == n_clipped, (what, info, want[1:])


def signals(ceiling, shift):
    """one seeded signal per length; the peaks lie below, exactly at and above the ceiling, one stream holds only
    subnormals and one runs from 1 down through every exponent to the subnormals; `shift` rotates the kinds over the lengths"""
    rng = np.random.default_rng([0x1E7, shift])
    c = float(ceiling)
    kinds = ["at", "below", "above", "subnormal", "at", "far_above", "decay"]
    out = []
    for j, n in enumerate(LENGTHS):
        kind = kinds[(j + shift) % len(kinds)]
        x = rng.uniform(-1, 1, n)
        if kind == "subnormal":
            x = rng.integers(-(1 << 22), 1 << 22, n).astype(np.float64) * TINY
        elif kind == "decay":
            x = x * np.exp(-100.0 * np.arange(n) / max(n - 1, 1))
        elif n:
            top = {"at": c, "below": 0.6 * c, "above": min(1.7 * c, 0.999), "far_above": 40.0}[kind]
            x = x * (0.98 * top)
            x[int(rng.integers(n))] = top * rng.choice([-1.0, 1.0])
        out.append(np.asarray(x, F32))
    return out


MODES = [LR.Level(mode, flags, gain, ceiling)
         for mode, gain, ceiling in ((LEVEL_GAIN, 0.75, 0.5), (LEVEL_GAIN, 1.9, 0.5), (LEVEL_GAIN, 1.0, 0.5), (LEVEL_FIT, 1.0, 0.5),
                                     (LEVEL_FIT, 1.0, 1.0), (LEVEL_NORMALIZE, 1.0, 0.5), (LEVEL_NORMALIZE, 1.0, 0.8912509))
         for flags in (0, LEVEL_CLIP)]


@pytest.mark.parametrize("level", MODES, ids=lambda l: "mode%d-clip%d-g%g-c%g" % l)
def test_level_streams_every_mode(gpu_ctx, level):
    n_clipped = 0
    for shift in range(3):
        pcm = signals(level.ceiling, shift)
        got, info = gpu_ctx.level_streams(pcm, lv(level))
        assert [len(y) for y in got] == LENGTHS and len(info) == len(LENGTHS)
        for i, (x, y) in enumerate(zip(pcm, got)):
            want = LR.apply(x, level, FLT_MAX)
            assert same_bits(y, want[0]), (shift, i)
            check_info(info[i], want, (shift, i))
            assert info[i]["mode"] == level.mode
            n_clipped += want[4]
            if level.mode == LEVEL_FIT and want[1] <= F32(level.ceiling):
                assert want[2] == 1 and same_bits(y, x)
    # the clamp has something to do exactly where a plain gain leaves a peak above the ceiling
    assert (n_clipped > 0) == (level.mode == LEVEL_GAIN and bool(level.flags))


def test_level_streams_one_level_per_stream(gpu_ctx):
    pcm = signals(0.5, 1)
    pcm[6] = (np.random.default_rng(6).uniform(-1, 1, 4097) * 1e-3).astype(F32)
    levels = [LR.Level(LEVEL_FIT, 0, 1.0, 0.25), LR.Level(LEVEL_GAIN, LEVEL_CLIP, 3.0, 0.25), LR.Level(LEVEL_NORMALIZE, 0, 1.0, 1.0),
              LR.Level(LEVEL_GAIN, 0, 0.3333, 1.0), LR.Level(LEVEL_FIT, LEVEL_CLIP, 1.0, 0.5), LR.Level(LEVEL_NORMALIZE, LEVEL_CLIP, 1.0, 0.1),
              LR.Level(LEVEL_GAIN, 0, 1e-38, 1.0)]          # the last one's products are all subnormal
    got, info = gpu_ctx.level_streams(pcm, [lv(l) for l in levels])
    for i, (x, y, l) in enumerate(zip(pcm, got, levels)):
        want = LR.apply(x, l, FLT_MAX)
        assert same_bits(y, want[0]), i
        check_info(info[i], want, i)
        assert info[i]["mode"] == l.mode
    sub = np.abs(got[6]) < np.finfo(F32).tiny
    assert sub.all() and (got[6] != 0).any()
    # int16 input is divided by 32768 first, as the encoders take it
    x16 = np.array([-32768, 5, 32767, -7], np.int16)
    got, info = gpu_ctx.level_streams([x16], Level(LEVEL_FIT, ceiling=0.5))
    want = LR.apply(x16.astype(F32) / F32(32768), LR.Level(LEVEL_FIT, 0, 1.0, 0.5), FLT_MAX)
    assert same_bits(got[0], want[0]) and info[0]["peakIn"] == 1.0


def fit_gains(P, c):
    """level_ref.fit_gain over an array of peaks > 0"""
    g = (c / P).astype(F32)
    g[np.isinf(g)] = F32(FLT_MAX)
    for _ in range(4):
        over = (P * g).astype(F32) > c
        g[over] = np.nextafter(g[over], F32(0))
    assert not ((P * g).astype(F32) > c).any()
    return g


def test_level_streams_more_streams_than_a_grid_has_rows(gpu_ctx):
    """65 537 streams of one to three samples; FIT to 0.5 gives every stream its own gain, and the streams past the 65 535th,
    which a block reaches only by striding, peak above the ceiling"""
    n = 65537
    rng = np.random.default_rng(0x10001)
    lens = 1 + (np.arange(n) % 3)
    offs = np.concatenate([[0], np.cumsum(lens)])
    flat = rng.uniform(-1, 1, offs[-1]).astype(F32)
    flat[offs[-4]:] = np.array([0.9, -0.7, 0.2, 0.6, -0.95, 0.8, 0.1][-(offs[-1] - offs[-4]):], F32)
    pcm = [flat[offs[i]:offs[i + 1]] for i in range(n)]
    c = F32(0.5)
    got, info = gpu_ctx.level_streams(pcm, Level(LEVEL_FIT, ceiling=0.5))
    P = np.maximum.reduceat(np.abs(flat), offs[:-1])
    g = np.ones(n, F32)
    g[P > c] = fit_gains(P[P > c], c)
    assert np.array_equal(info["peakIn"].view(np.uint32), P.view(np.uint32))
    assert np.array_equal(info["gain"].view(np.uint32), g.view(np.uint32))
    assert np.array_equal(info["peakOut"].view(np.uint32), (P * g).astype(F32).view(np.uint32))
    assert not info["nClipped"].any() and (info["mode"] == LEVEL_FIT).all()
    assert same_bits(np.concatenate(got), (flat * np.repeat(g, lens)).astype(F32))
    assert (g[-3:] < 1).all() and (g == 1).sum() > 1000 and (g < 1).sum() > 1000
    for i in list(range(0, 40)) + list(range(n - 40, n)):
        want = LR.apply(pcm[i], LR.Level(LEVEL_FIT, 0, 1.0, 0.5), FLT_MAX)
        assert same_bits(got[i], want[0])
        check_info(info[i], want, i)
    # a clamp across the same streams: the counts are per stream
    got, info = gpu_ctx.level_streams(pcm, Level(LEVEL_GAIN, LEVEL_CLIP, 1.5, 0.5))
    scaled = (flat * F32(1.5)).astype(F32)
    over = np.abs(scaled) > c
    assert same_bits(np.concatenate(got), np.where(over, np.copysign(c, scaled), scaled).astype(F32))
    assert np.array_equal(info["nClipped"], np.add.reduceat(over.astype(np.uint64), offs[:-1]))


def test_level_streams_refusals(gpu_ctx):
    L, h = gpu_ctx.L, gpu_ctx.h
    msg = lambda: L.dcs_last_error(h).decode()
    good = [np.full(5, 0.25, F32), np.full(3, 0.5, F32)]
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(DcsError) as e:
            gpu_ctx.level_streams([good[0], np.array([0.1, bad, 0.2], F32)], Level(LEVEL_FIT))
        assert e.value.status == ERR_BAD_STREAM and msg().startswith("stream 1:") and "not finite" in msg()
    with pytest.raises(DcsError) as e:                      # a plain gain that overflows, not clamped
        gpu_ctx.level_streams([good[0], np.full(3, 3e38, F32)], Level(LEVEL_GAIN, gain=2.0))
    assert e.value.status == ERR_BAD_STREAM and msg().startswith("stream 1:")
    got, info = gpu_ctx.level_streams([np.full(3, 3e38, F32)], Level(LEVEL_GAIN, LEVEL_CLIP, 2.0, 1.0))     # clamped: accepted
    assert list(got[0]) == [1.0] * 3 and info[0]["nClipped"] == 3 and info[0]["peakOut"] == 1.0
    for i, bad in enumerate([Level(0), Level(LEVEL_FIT, 2), Level(LEVEL_GAIN, gain=0.0), Level(LEVEL_FIT, ceiling=1.5)]):
        levels = [Level(LEVEL_FIT), Level(LEVEL_FIT)]
        levels[i % 2] = bad
        with pytest.raises(DcsError) as e:
            gpu_ctx.level_streams(good, levels)
        assert e.value.status == ERR_INVALID_ARG and msg().startswith("stream %d:" % (i % 2)), msg()
    # nLevels is 1 or nStreams; levels are required
    pcm = np.concatenate(good + [good[0]])
    offs = np.array([0, 5, 8, 13], np.uint64)
    out, out_offs = np.zeros(13, F32), np.zeros(4, np.uint64)
    two = (Level * 2)(Level(LEVEL_FIT), Level(LEVEL_FIT))
    for levels, n_levels in ((two, 2), (two, 0), (None, 1), (None, 0)):
        assert L.dcs_level_streams(h, _ptr(pcm), _ptr(offs), 3, levels, n_levels, _ptr(out), 13, _ptr(out_offs), None) == ERR_INVALID_ARG
    assert L.dcs_level_streams(h, _ptr(pcm), _ptr(offs), 3, two, 1, _ptr(out), 12, _ptr(out_offs), None) == -5      # capacity
    assert list(out_offs) == [0, 5, 8, 13]
    got, info = gpu_ctx.level_streams([], Level(LEVEL_FIT))
    assert got == [] and len(info) == 0


# ------------------------------------------------------------------------------------------------- after the converter

SQUARE = np.where((np.arange(1200) // 50) & 1, -1.0, 1.0).astype(F32)       # full scale, period 100 samples
NOISE = np.random.default_rng(5).uniform(-0.4, 0.4, 500).astype(F32)
# (name, values, rate, channels)
PLAIN = [("square_44100_stereo", np.repeat(SQUARE, 2), 44100, 2), ("noise_8000", NOISE, 8000, 1),
         ("square_31250_pass", SQUARE[:700] * F32(0.95), 31250, 1), ("square_48000", SQUARE, 48000, 1)]
UNITY = [("square_31250_unity", SQUARE[:900], 31250, 1), ("noise_8000", NOISE, 8000, 1)]
_RESAMPLED = {}


def resampled(cases, at_unity):
    """resample_ref's floats for each case, computed once"""
    c, inc = rs_cases.tables()["default"]
    out = []
    for name, x, rate, ch in cases:
        key = (name, at_unity)
        if key not in _RESAMPLED:
            y = RS.resample(x, rate, c, inc, ch, RS.AT_UNITY if at_unity else 0)
            y.setflags(write=False)
            _RESAMPLED[key] = y
        out.append(_RESAMPLED[key])
    return out


def test_the_inputs_take_both_branches_of_fit():
    peaks = [float(np.abs(y).max()) for y in resampled(PLAIN, False) + resampled(UNITY, True)]
    assert [F32(p) for p in peaks] == [F32(1.2161008), F32(0.58210206), F32(0.95), F32(1.2098658), F32(1.0872074), F32(0.58210206)]


@pytest.mark.parametrize("cases,at_unity", [(PLAIN, False), (UNITY, True)], ids=["plain", "at_unity"])
def test_resample_streams_with_level(gpu_ctx, cases, at_unity):
    ys = resampled(cases, at_unity)
    pcm, rates, chans = [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases]
    plain = gpu_ctx.resample_streams(pcm, rates, chans, at_unity=at_unity)
    assert isinstance(plain, list) and all(same_bits(a, b) for a, b in zip(plain, ys))
    n = len(cases)
    per_stream = [LR.Level(LEVEL_FIT, 0, 1.0, 0.8912509), LR.Level(LEVEL_NORMALIZE, 0, 1.0, 1.0), LR.Level(LEVEL_GAIN, LEVEL_CLIP, 1.25, 0.9),
                  LR.Level(LEVEL_GAIN, 0, 0.5, 1.0)][:n]
    for levels in ([LR.Level(LEVEL_FIT, 0, 1.0, 1.0)] * n, [LR.Level(LEVEL_FIT, LEVEL_CLIP, 1.0, 0.8912509)] * n,
                   [LR.Level(LEVEL_GAIN, LEVEL_CLIP, 1.0, 1.0)] * n, per_stream):
        arg = lv(levels[0]) if levels[0] == levels[-1] else [lv(l) for l in levels]
        got, info = gpu_ctx.resample_streams(pcm, rates, chans, at_unity=at_unity, level=arg)
        for i in range(n):
            want = LR.apply(ys[i], levels[i], FLT_MAX)
            assert same_bits(got[i], want[0]), (cases[i][0], levels[i])
            check_info(info[i], want, (cases[i][0], levels[i]))
            if want[2] == 1 and not want[4]:
                assert same_bits(got[i], plain[i])
    # FIT to 1 scaled the loud ones and nothing else
    got, info = gpu_ctx.resample_streams(pcm, rates, chans, at_unity=at_unity, level=Level(LEVEL_FIT))
    assert [bool(g < 1) for g in info["gain"]] == [bool(np.abs(y).max() > 1) for y in ys]
    assert (info["peakOut"] <= 1).all() and any(info["gain"] < 1) and any(info["gain"] == 1)


@pytest.mark.parametrize("version", [0x9400, 0x9302])
def test_encode_streams_at_with_fit(gpu_ctx, version):
    ys = resampled(PLAIN, False)
    pcm, rates, chans = [c[1] for c in PLAIN], [c[2] for c in PLAIN], [c[3] for c in PLAIN]
    fit = LR.Level(LEVEL_FIT, 0, 1.0, 1.0)
    leveled = [LR.apply(y, fit, 1.0) for y in ys]
    out, info, linfo = gpu_ctx.encode_streams_at(pcm, rates, version, channels=chans, level=lv(fit))
    want, winfo = gpu_ctx.encode_streams([w[0] for w in leveled]) if version == 0x9400 else gpu_ctx.encode93_streams([w[0] for w in leveled], D.OS93B)
    assert out == want and [tuple(a) for a in info] == [tuple(b) for b in winfo]
    for i in range(len(PLAIN)):
        check_info(linfo[i], leveled[i], PLAIN[i][0])
    assert [bool(g < 1) for g in linfo["gain"]] == [True, False, False, True]
    for i in (0, 3):                        # the two scaled ones against the encoders' restatements as well
        ref = E.encode(leveled[i][0])[0] if version == 0x9400 else E93.encode(leveled[i][0], version)[0]
        assert out[i] == ref, PLAIN[i][0]
    # without a level the loud streams are refused as ever, and a level whose gain comes out 1 changes no byte
    with pytest.raises(DcsError) as e:
        gpu_ctx.encode_streams_at(pcm, rates, version, channels=chans)
    msg = gpu_ctx.L.dcs_last_error(gpu_ctx.h).decode()
    assert e.value.status == ERR_BAD_STREAM and msg.startswith("stream 0:") and "peaks at |x| = 1.21610" in msg
    quiet = gpu_ctx.encode_streams_at(pcm[1:3], rates[1:3], version, channels=chans[1:3])
    for level in (Level(LEVEL_FIT), Level(LEVEL_GAIN, gain=1.0), Level(LEVEL_GAIN, LEVEL_CLIP, 1.0, 1.0), [Level(LEVEL_FIT), Level(LEVEL_FIT, ceiling=0.96)]):
        o, inf, li = gpu_ctx.encode_streams_at(pcm[1:3], rates[1:3], version, channels=chans[1:3], level=level)
        assert o == quiet[0] and [tuple(a) for a in inf] == [tuple(b) for b in quiet[1]]
        assert list(li["gain"]) == [1.0, 1.0] and not li["nClipped"].any()
        assert list(li["peakIn"]) == list(li["peakOut"]) == [F32(0.58210206), F32(0.95)]


def test_encode_streams_at_gain_beyond_one_is_refused(gpu_ctx):
    pcm, rates = [NOISE, SQUARE[:700] * F32(0.95)], [8000, 31250]
    with pytest.raises(DcsError) as e:
        gpu_ctx.encode_streams_at(pcm, rates, level=Level(LEVEL_GAIN, gain=1.5))
    msg = gpu_ctx.L.dcs_last_error(gpu_ctx.h).decode()
    assert e.value.status == ERR_BAD_STREAM and msg.startswith("stream 1:") and "peaks at |x| = 1.42499" in msg, msg
    # clamped, it is encoded: the bytes of the clamped signal
    level = LR.Level(LEVEL_GAIN, LEVEL_CLIP, 1.5, 1.0)
    out, _, li = gpu_ctx.encode_streams_at(pcm, rates, level=lv(level))
    ys = resampled([PLAIN[1], PLAIN[2]], False)
    want = [LR.apply(y, level, 1.0) for y in ys]
    assert out == gpu_ctx.encode_streams([w[0] for w in want])[0]
    for i in range(2):
        check_info(li[i], want[i], i)
    assert li[1]["nClipped"] == 700 and li[0]["nClipped"] == 0
    with pytest.raises(DcsError) as e:                      # a bad level names its stream before anything runs
        gpu_ctx.encode_streams_at(pcm, rates, level=[Level(LEVEL_FIT), Level(7)])
    assert e.value.status == ERR_INVALID_ARG and gpu_ctx.L.dcs_last_error(gpu_ctx.h).decode().startswith("stream 1:")


# ---------------------------------------------------------------------------------------------------------------- files

def dcsa(fmt, frames, seed):
    s = D.synth_stream(fmt, frames, seed=seed)
    return D.dcsa_header(D.format_os(fmt), len(s)) + s


def restated_file(data, flac, at_unity, level, bound):
    """a file's samples as the encoder reads them after the stage: the restated reader, converter and level"""
    st, mono, d = (FR if flac else WR).decode(data)
    assert st == 0
    c, inc = rs_cases.tables()["default"]
    y = RS.convert(mono, d["rate"], c, inc, RS.AT_UNITY if at_unity else 0)
    return LR.apply(y, level, bound)


def test_encode_files_with_fit(gpu_ctx):
    """the call test_full_scale_negative_is_accepted shows refused encodes both files once FIT is asked for"""
    wav = dict(WC.cases())
    files = [wav["s16_1ch_22050"], wav["fullscale_s16_31250"]]
    with pytest.raises(DcsError) as e:
        gpu_ctx.encode_files(files, at_unity=True)
    assert e.value.status == ERR_BAD_STREAM
    fit = LR.Level(LEVEL_FIT, 0, 1.0, 1.0)
    b16 = float(F32(32768) / F32(32767))
    out, info, li = gpu_ctx.encode_files(files, at_unity=True, level=lv(fit))
    assert li[1]["peakIn"] > 1 and li[1]["gain"] < 1 and li[1]["peakOut"] <= 1
    assert li[0]["gain"] == 1 and out[0] == gpu_ctx.encode_files(files[:1], at_unity=True)[0][0]
    want = [restated_file(f, False, True, fit, b16) for f in files]
    assert F32(want[1][1]) == F32(1.0443262)
    for i in range(2):
        check_info(li[i], want[i], i)
        assert li[i]["mode"] == LEVEL_FIT
    assert out[1] == gpu_ctx.encode_streams([want[1][0]])[0][0]
    assert list(info["kind"]) == [D.FILE_WAV] * 2 and info[1]["nSamples"] == len(want[1][0])


def test_encode_files_with_fit_flac_and_dcsa(gpu_ctx):
    wav, flac = dict(WC.cases()), dict(FC.cases())
    box = dcsa(D.FMT_94_T0, 40, 1)
    files = [wav["s16_1ch_22050"], box, flac["fullscale_s16_31250"], wav["fullscale_s16_31250"]]
    is_flac = [False, None, True, False]
    fit = LR.Level(LEVEL_FIT, 0, 1.0, 1.0)
    b16 = float(F32(32768) / F32(32767))
    for at_unity in (False, True):
        out, info, li = gpu_ctx.encode_files(files, at_unity=at_unity, level=lv(fit))
        assert list(info["kind"]) == [D.FILE_WAV, D.FILE_DCSA_COPY, D.FILE_FLAC, D.FILE_WAV]
        # the container: the neutral record, and the bytes of the call without a level
        assert tuple(li[1]) == (0.0, 1.0, 0.0, 0, 0) and out[1] == gpu_ctx.encode_files([box])[0][0] == box[36:]
        for i in (0, 2, 3):
            want = restated_file(files[i], is_flac[i], at_unity, fit, b16)
            check_info(li[i], want, (at_unity, i))
            assert out[i] == gpu_ctx.encode_streams([want[0]])[0][0], (at_unity, i)
        # passed through, both full-scale files hold -32768 / 32767 and are scaled; through the converter the FLAC file's
        # alternating samples come out at 0.7962882 and are left alone, the WAV file's step overshoots
        assert li[0]["gain"] == 1
        assert (li[2]["peakIn"] == F32(0.7962882) and li[2]["gain"] == 1) if at_unity else (li[2]["peakIn"] == F32(b16) and li[2]["gain"] < 1)
        assert li[3]["gain"] < 1 and li[3]["peakOut"] <= 1
        if at_unity:
            assert out[2] == gpu_ctx.encode_files([files[2]], at_unity=True)[0][0]
    # one level per file: the container's is checked like the others, and ignored
    levels = [Level(LEVEL_FIT), Level(LEVEL_GAIN, gain=0.5), Level(LEVEL_GAIN, gain=0.5), Level(LEVEL_GAIN, LEVEL_CLIP, 2.0, 0.25)]
    out, info, li = gpu_ctx.encode_files(files, level=levels)
    assert tuple(li[1]) == (0.0, 1.0, 0.0, 0, 0) and out[1] == box[36:]
    want = restated_file(files[3], False, False, LR.Level(LEVEL_GAIN, LEVEL_CLIP, 2.0, 0.25), b16)
    check_info(li[3], want, 3)
    assert want[4] > 0 and out[3] == gpu_ctx.encode_streams([want[0]])[0][0]
    levels[1] = Level(LEVEL_GAIN, gain=-1.0)
    with pytest.raises(DcsError) as e:
        gpu_ctx.encode_files(files, level=levels)
    assert e.value.status == ERR_INVALID_ARG and gpu_ctx.L.dcs_last_error(gpu_ctx.h).decode().startswith("file 1:")
    # a plain gain that leaves a file beyond its format's full scale is refused with the file encoder's message
    with pytest.raises(DcsError) as e:
        gpu_ctx.encode_files(files, level=[Level(LEVEL_FIT), Level(LEVEL_FIT), Level(LEVEL_GAIN, gain=1.01), Level(LEVEL_FIT)])
    msg = gpu_ctx.L.dcs_last_error(gpu_ctx.h).decode()
    assert e.value.status == ERR_BAD_STREAM and msg.startswith("file 2:") and "peaks at" in msg and "beyond" in msg
