"""Seeded cases of the rate-distortion 1994+ encoder (test infrastructure): the signals, the (signal, layout, budget, error
floor) grid the host and the GPU tests share, and the restatement's result for each, computed once per process."""
import functools

import numpy as np

import enc94rd_ref as R
import sweep_ref as S

F32 = np.float32
MQE = R.DEFAULTS["maximumQuantizationError"]


def _t(n):
    return np.arange(n) / 31250.0


def _signals():
    rng = np.random.default_rng(0x94D0)
    out = {}
    out["silence"] = np.zeros(240 * 2, F32)
    out["dc"] = np.full(240 * 2 - 7, 0.25, F32)
    out["sine_fs"] = np.sin(2 * np.pi * 997.0 * _t(240 * 33)).astype(F32)
    out["noise_m40"] = (rng.normal(0, 0.01, 240 * 17)).clip(-1, 1).astype(F32)
    x = np.zeros(240 * 3, F32)
    x[239], x[240] = 0.9, -0.9
    out["impulse_edge"] = x
    out["band15"] = (0.5 * np.sin(2 * np.pi * 15000.0 * _t(240 * 17 - 100))).astype(F32)
    out["bands012"] = (0.6 * np.sin(2 * np.pi * 700.0 * _t(240 * 33 - 1)) * (0.55 + 0.45 * np.sin(2 * np.pi * 9.0 * _t(240 * 33 - 1)))).astype(F32)
    x = (rng.normal(0, 0.2, 240 * 3)).clip(-1, 1).astype(F32)
    x[:240] *= F32(0.001)
    out["level_step"] = x
    out["one_frame"] = (rng.normal(0, 0.3, 200)).clip(-1, 1).astype(F32)
    m = (0.4 * np.sin(2 * np.pi * 220.0 * _t(240 * 17)) + 0.2 * np.sin(2 * np.pi * 3300.0 * _t(240 * 17))
         + rng.normal(0, 0.02, 240 * 17)) * np.linspace(1.0, 0.05, 240 * 17)
    out["music"] = m.clip(-1, 1).astype(F32)
    out["tone4k"] = (0.999 * np.sin(2 * np.pi * 4000.0 * _t(240 * 3))).astype(F32)
    out["tone9k"] = (0.999 * np.sin(2 * np.pi * 9000.0 * _t(240 * 3))).astype(F32)
    # a near-silent first frame, then a band louder than any code but 15 can hold at header code 0: the step 0 -> 15 has no
    # delta code, so only a chain whose first frame needs little takes the widest option afterwards
    n = 240 * 4
    gate = np.where(np.arange(n) < 240, 0.0005, 1.0)
    out["step_dc"] = np.where(np.arange(n) < 240, 0.0005 * rng.normal(0, 1, n), 0.99).astype(F32)
    out["step_sq4k"] = (gate * 0.999 * np.sign(np.sin(2 * np.pi * 3900.0 * _t(n)))).astype(F32)
    out["step_t9k"] = (gate * 0.999 * np.sin(2 * np.pi * 9000.0 * _t(n))).astype(F32)
    out["step_sq9k"] = (gate * 0.999 * np.sign(np.sin(2 * np.pi * 7800.0 * _t(n)))).astype(F32)
    return out


SIGNALS = _signals()
FRAMES = {n: (len(x) + 239) // 240 for n, x in SIGNALS.items()}
assert set(FRAMES.values()) >= {1, 2, 3, 17, 33}
FMTS = {"T0": (0, 0), "T0s3": (0, 3), "T1s0": (1, 0), "T1s3": (1, 3), "wild": (-1, -1), "T1": (1, -1)}
# (signal, layout, targetBitRate, maximumQuantizationError)
GRID = [
    ("silence", "wild", 128000, MQE), ("dc", "T0", 128000, MQE), ("dc", "T1s3", 64000, 0.0),
    ("sine_fs", "T0", 256000, 0.0), ("sine_fs", "T1s0", 128000, MQE), ("sine_fs", "T1s3", 48000, MQE),
    ("noise_m40", "T0s3", 96000, 0.0), ("noise_m40", "T1s3", 1000000, 0.0), ("noise_m40", "wild", 64000, MQE),
    ("impulse_edge", "T0", 128000, 0.0), ("impulse_edge", "T1", 128000, MQE),
    ("band15", "T0", 2000000, 0.0), ("band15", "T1s0", 64000, MQE), ("band15", "T1s3", 192000, 0.0),
    ("bands012", "T0", 16000, 0.0), ("bands012", "T1s0", 256000, 0.0), ("bands012", "T1s3", 256000, 0.0), ("bands012", "T1s3", 24000, MQE),
    ("level_step", "T0", 128000, MQE), ("level_step", "T1s0", 400000, 0.0), ("level_step", "T1s3", 400000, 0.0),
    ("one_frame", "wild", 128000, MQE), ("one_frame", "T0", 1, 0.0), ("one_frame", "T1s0", 1, MQE),
    ("music", "T0", 2000000, 0.0), ("music", "T1s3", 96000, MQE), ("music", "wild", 32000, MQE), ("music", "T1s0", 2000000, 0.0),
    ("one_frame", "T1s3", 2000000, 0.0), ("tone4k", "T1s3", 5000000, 0.0), ("tone9k", "T1s0", 5000000, 0.0),
    ("step_dc", "T1s0", 100000, 0.0), ("step_dc", "T1s3", 5000000, MQE), ("step_sq4k", "T1s3", 5000000, MQE),
    ("step_sq4k", "T1s0", 100000, 0.0), ("step_t9k", "T1s0", 100000, 0.0), ("step_sq9k", "T1s3", 100000, MQE),
]
IDS = ["%s-%s-%d-%s" % (n, f, r, "q0" if q == 0 else "qd") for n, f, r, q in GRID]


@functools.lru_cache(maxsize=None)
def analysis(name):
    return R.analyse(SIGNALS[name])


@functools.lru_cache(maxsize=None)
def expected(name, fmt, rate, mqe, budget_bytes=None):
    """-> (stream bytes, info dict, reconstruction, codes)"""
    return R.encode(analysis(name), FMTS[fmt], budget_bytes, targetBitRate=rate, maximumQuantizationError=mqe)


def params(rate, mqe):
    return dict(targetBitRate=rate, maximumQuantizationError=mqe)


def info_tuple(ch):
    return (ch["type"], ch["sub"], ch["ladderIndex"], ch["numBands"], ch["frameBits"], ch["budgetBits"], ch["sqErr"], int(ch["fits"]))


def info_of(rec):
    """an ENCODE_RD_INFO_DTYPE record as info_tuple gives it"""
    return tuple(int(rec[k]) for k in ("formatType", "formatSubType", "ladderIndex", "numBands", "frameBits", "budgetBits", "sqErr", "fits"))


def closing_probe(stream, ch, codes):
    """the stream with one frame more, in which every kept band returns to code 0 (a delta code each, no samples), so that a
    decoder asked for that frame too shows where the last real frame ended: the real stream's bits are a prefix of this one.
    (Decoding one frame past a 1994+ stream instead would read band-type deltas out of whatever follows.)"""
    F = (stream[0] << 8) | stream[1]
    bits = np.unpackbits(np.frombuffer(stream[18:], np.uint8))[:ch["frameBits"]]
    extra = []
    for b in range(ch["numBands"]):
        d = 16 - int(codes[-1, b])
        extra += [(int(R.E.HDR_CODE[d]) >> (int(R.HL[d]) - 1 - k)) & 1 for k in range(int(R.HL[d]))]
    body = np.packbits(np.concatenate([bits, np.array(extra, np.uint8)])).tobytes()
    return bytes([(F + 1) >> 8, (F + 1) & 0xFF]) + stream[2:18] + body + bytes(8)


def time_error(oracle, os_, x, stream):
    """sweep_ref.measure's squared error of a stream decoded by the oracle from a fresh decoder at unity"""
    nf = (stream[0] << 8) | stream[1]
    return S.sq_err(S.measure(x, oracle.decode(os_, 255, [stream], [255], nf + 1)))


# the quality condition: the recordings whose source PCM tests/golden/encoder_golden.npz carries, and seeded signals of
# tests/enc_cases.py, each cut to at most 64 frames; the layouts; the rates are sweep_ref.RATES
QUALITY_FRAMES = 64
QUALITY_LAYOUTS = [(0, 0), (1, 0), (1, 3)]
QUALITY_SEEDED = ["ec_music0", "ec_music1", "ec_square"]
QUALITY_GPU = ["rec:ENC-94-T0-v0", "rec:ENC-93b-T1-v0", "ec_music0", "ec_square"]       # the four checked on the device's own bytes


@functools.lru_cache(maxsize=None)
def quality_signals():
    """{name: PCM}"""
    import os
    import enc_cases as EC
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz"))
    out = {"rec:" + k[:-4]: z[k].reshape(-1)[:240 * QUALITY_FRAMES] for k in z.files if k.endswith("/pcm")}
    out["ec_music0"] = EC._music(np.random.default_rng([0x94D2, 0]), 240 * 40).astype(F32)
    out["ec_music1"] = EC._music(np.random.default_rng([0x94D2, 1]), 240 * 24 - 77).astype(F32)
    out["ec_square"] = (EC._square(np.random.default_rng([0x94D2, 2]), 240 * 12) * F32(0.5)).astype(F32)
    return out


@functools.lru_cache(maxsize=None)
def quality_analysis(name):
    return R.analyse(quality_signals()[name])


def quality_reference(oracle, name, lay, rate, stream=None):
    """(B, E) of the reference-equal stream (enc_ref's, or `stream`) of one quality case"""
    x = quality_signals()[name]
    if stream is None:
        stream = R.E.encode(x, lay, targetBitRate=rate)[0]
    return len(stream), time_error(oracle, 3 if lay[1] == 3 else 2, R.E.to_float(x), stream)
