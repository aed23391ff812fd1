"""Seeded cases of the rate-distortion OS93 Type-0 encoder (test infrastructure): the signals, the (signal, version, budget,
error floor) grid the host and the GPU tests share, and the restatement's result for each, computed once per process."""
import functools

import numpy as np

import enc93rd_ref as R
import sweep_ref as S

F32 = np.float32
MQE = R.DEFAULTS["maximumQuantizationError"]
A, B = 0x9301, 0x9302


def _t(n):
    return np.arange(n) / 31250.0


def _signals():
    rng = np.random.default_rng(0x93D0)
    out = {}
    out["silence"] = np.zeros(240 * 2, F32)
    out["tone700"] = (0.6 * np.sin(2 * np.pi * 700.0 * _t(240 * 33 - 1)) * (0.55 + 0.45 * np.sin(2 * np.pi * 9.0 * _t(240 * 33 - 1)))).astype(F32)
    out["sine_fs"] = np.sin(2 * np.pi * 997.0 * _t(240 * 17)).astype(F32)
    out["square_fs"] = np.sign(np.sin(2 * np.pi * 1234.0 * _t(240 * 3 - 5))).astype(F32)
    out["noise_m40"] = (rng.normal(0, 0.01, 240 * 17)).clip(-1, 1).astype(F32)
    x = np.zeros(240 * 3, F32)
    x[239], x[240] = 0.9, -0.9
    out["impulse_edge"] = x
    out["band15"] = (0.5 * np.sin(2 * np.pi * 15200.0 * _t(240 * 17 - 100))).astype(F32)
    x = (rng.normal(0, 0.2, 240 * 3)).clip(-1, 1).astype(F32)
    x[:240] *= F32(0.001)
    out["level_step"] = x
    out["one_frame"] = (rng.normal(0, 0.3, 200)).clip(-1, 1).astype(F32)
    m = (0.4 * np.sin(2 * np.pi * 220.0 * _t(240 * 17)) + 0.2 * np.sin(2 * np.pi * 3300.0 * _t(240 * 17))
         + rng.normal(0, 0.02, 240 * 17)) * np.linspace(1.0, 0.05, 240 * 17)
    out["music"] = m.clip(-1, 1).astype(F32)
    out["dc"] = np.full(240 * 2 - 7, 0.25, F32)
    # bands 4..7 alone: zero bands before and behind coded ones
    out["mid_tone"] = (0.3 * np.sin(2 * np.pi * 5400.0 * _t(240 * 3)) + 0.25 * np.sin(2 * np.pi * 6900.0 * _t(240 * 3))).astype(F32)
    return out


SIGNALS = _signals()
FRAMES = {n: (len(x) + 239) // 240 for n, x in SIGNALS.items()}
assert set(FRAMES.values()) >= {1, 2, 3, 17, 33}
# (signal, formatVersion, targetBitRate, maximumQuantizationError)
GRID = [
    ("silence", A, 128000, MQE), ("silence", B, 128000, 0.0),
    ("tone700", A, 16000, 0.0), ("tone700", B, 256000, MQE), ("tone700", B, 24000, MQE),
    ("sine_fs", A, 256000, 0.0), ("sine_fs", B, 48000, MQE), ("sine_fs", B, 5000000, 0.0),
    ("square_fs", A, 128000, MQE), ("square_fs", B, 5000000, 0.0),
    ("noise_m40", A, 96000, 0.0), ("noise_m40", B, 1000000, 0.0), ("noise_m40", B, 64000, MQE),
    ("impulse_edge", A, 128000, 0.0), ("impulse_edge", B, 128000, MQE), ("impulse_edge", B, 5000000, 0.0),
    ("band15", A, 2000000, 0.0), ("band15", B, 64000, MQE),
    ("level_step", A, 128000, MQE), ("level_step", B, 400000, 0.0),
    ("one_frame", A, 128000, MQE), ("one_frame", A, 1, 0.0), ("one_frame", B, 1, MQE), ("one_frame", B, 2000000, 0.0),
    ("music", A, 2000000, 0.0), ("music", B, 96000, MQE), ("music", B, 32000, MQE), ("music", A, 12000, 0.0),
    ("dc", A, 128000, MQE), ("dc", B, 64000, 0.0),
    ("mid_tone", A, 64000, MQE), ("mid_tone", B, 400000, 0.0),
]
IDS = ["%s-%x-%d-%s" % (n, v, r, "q0" if q == 0 else "qd") for n, v, r, q in GRID]


@functools.lru_cache(maxsize=None)
def analysis(name, version):
    return R.analyse(SIGNALS[name], version)


@functools.lru_cache(maxsize=None)
def expected(name, version, rate, mqe, budget_bytes=None):
    """-> (stream bytes, info dict, reconstruction, states)"""
    return R.encode(analysis(name, version), budget_bytes, targetBitRate=rate, maximumQuantizationError=mqe)


def params(rate, mqe):
    return dict(targetBitRate=rate, maximumQuantizationError=mqe)


def info_tuple(ch):
    return (ch["type"], ch["sub"], ch["ladderIndex"], ch["numBands"], ch["frameBits"], ch["budgetBits"], ch["sqErr"], int(ch["fits"]))


def info_of(rec):
    """an ENCODE_RD_INFO_DTYPE record as info_tuple gives it"""
    return tuple(int(rec[k]) for k in ("formatType", "formatSubType", "ladderIndex", "numBands", "frameBits", "budgetBits", "sqErr", "fits"))


def fnv1a64(b):
    h = 0xCBF29CE484222325
    for v in b:
        h = ((h ^ v) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def time_error(oracle, version, x, stream):
    """sweep_ref.measure's squared error of a stream decoded by the oracle from a fresh decoder at unity"""
    nf = (stream[0] << 8) | stream[1]
    return S.sq_err(S.measure(x, oracle.decode(R.OS_OF[version], 255, [stream], [255], nf + 1)))


# the quality condition: the recordings whose source PCM tests/golden/encoder_golden.npz carries, and seeded signals of
# tests/enc_cases.py, each cut to at most 64 frames; both versions; the rates are sweep_ref.RATES
QUALITY_FRAMES = 64
QUALITY_GPU = ["rec:ENC-93a-T0-v0", "rec:ENC-93b-T0-v0", "ec_music0", "ec_square"]      # the four checked on the device's own bytes


@functools.lru_cache(maxsize=None)
def quality_signals():
    """{name: PCM}"""
    import os
    import enc_cases as EC
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz"))
    out = {"rec:" + k[:-4]: z[k].reshape(-1)[:240 * QUALITY_FRAMES] for k in z.files if k.endswith("/pcm")}
    out["ec_music0"] = EC._music(np.random.default_rng([0x93D2, 0]), 240 * 40).astype(F32)
    out["ec_music1"] = EC._music(np.random.default_rng([0x93D2, 1]), 240 * 24 - 77).astype(F32)
    out["ec_square"] = (EC._square(np.random.default_rng([0x93D2, 2]), 240 * 12) * F32(0.5)).astype(F32)
    return out


@functools.lru_cache(maxsize=None)
def quality_analysis(name, version):
    return R.analyse(quality_signals()[name], version)
