"""The cases of the OS93a Type-1 encoder's tests (test infrastructure): seeded signals, the parameter grid, and the numpy
restatement's result for each (tests/enc93a_ref.py), computed once per process and shared by the host and the GPU tests."""
import hashlib
import os

import numpy as np

import enc93a_ref as A

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
RATES = [8000, 64000, A.DEFAULTS["targetBitRate"], 1000000]
MQES = [0.0, A.DEFAULTS["maximumQuantizationError"]]
TYPES = [1, -1]


def _signals():
    rng = np.random.default_rng(0x93A1)
    n = np.arange(240 * 5)
    out = {}
    rec = np.load(os.path.join(HERE, "golden", "encoder_golden.npz"))
    seen = set()
    for key in sorted(k for k in rec.files if k.endswith("/pcm")):
        x = np.ascontiguousarray(rec[key]).reshape(-1)
        mid = (len(x) // 480) * 240
        x = x[mid:mid + 6 * 240]                        # six frames from the middle of the recording
        h = hashlib.sha256(x.tobytes()).hexdigest()
        if h not in seen:
            seen.add(h)
            out["rec:" + key.split("/")[0]] = x
    out["silence"] = np.zeros(480, F32)
    out["len1"] = np.array([0.5], F32)
    out["len240"] = rng.uniform(-0.5, 0.5, 240).astype(F32)
    out["len241"] = rng.uniform(-0.5, 0.5, 241).astype(F32)
    out["len481"] = rng.uniform(-0.5, 0.5, 481).astype(F32)
    out["sine100_fs"] = np.sin(2 * np.pi * 100 * n / 31250).astype(F32)                 # band 0 at the largest scale
    out["noise_fs"] = rng.uniform(-1, 1, 240 * 4).astype(F32)                           # widths up to 9 under pp = 3
    # band 17 is pairs 114..126, frame-buffer words 228..253 of 256 over 0..15 625 Hz
    out["tone_band17"] = (0.5 * np.sin(2 * np.pi * (240.5 / 256 * 15625) * n / 31250)).astype(F32)
    out["noise_m60"] = (rng.standard_normal(240 * 3) * 1e-3).astype(F32)                # small scale codes
    out["dc"] = np.full(700, 0.25, F32)
    return out


SIGNALS = _signals()
NAMES = list(SIGNALS)
GRID = [(name, rate, mqe, typ) for name in NAMES for rate in RATES for mqe in MQES for typ in TYPES]
_AN, _RES = {}, {}


def params(rate, mqe):
    return dict(targetBitRate=int(rate), maximumQuantizationError=float(F32(mqe)))


def analysis(name):
    if name not in _AN:
        _AN[name] = A.analyse(SIGNALS[name])
    return _AN[name]


def type1(name, rate, mqe):
    """the restated Type-1 stream -> (bytes, info93a dict, reconstruction [F, 254])"""
    key = (name, rate, float(F32(mqe)))
    if key not in _RES:
        _RES[key] = A.encode_type1(analysis(name), **params(rate, mqe))
    return _RES[key]


def expected(name, rate, mqe, typ):
    """what encode93a_streams must return -> (bytes, type written, bandsToKeep, info93a dict)"""
    if typ == 1:
        s, ch, _ = type1(name, rate, mqe)
        return s, 1, ch["numBands"], ch
    key = (name, rate, float(F32(mqe)), "t0")
    if key not in _RES:
        _RES[key] = A.E93.encode(analysis(name)["x"], 0x9301, 0, **dict(A.DEFAULTS, **params(rate, mqe)))
    t0 = _RES[key]
    s, ch, _ = type1(name, rate, mqe)
    return (s, 1, ch["numBands"], ch) if len(s) < len(t0[0]) else (t0[0], 0, t0[2], ch)


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for x in bytes(data):
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h
