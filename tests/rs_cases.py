"""Seeded adversarial resampler cases, and the compiled libsamplerate as their checker (test infrastructure).

A case is one PCM stream with its rate, channel count, filter table and the at_unity flag.  Cases come in sets that share
table and flag, so a set is one dcs_resample_streams call.  Everything is a pure function of (seed, set index): a worker
process rebuilds a set from its key instead of receiving the samples.  Recipes only; no samples are committed.

The signals aim at where an f64 / f32 kernel parts from x86-64 SSE: f32 subnormal inputs and outputs, -0.0 beside +0.0,
normals just above 2^-126, noise that decays through the whole f32 range, values near FLT_MAX whose f64 sums round past it
when cast to f32, cancelling pairs, the int16 grid, 0.5 +- 1 ulp, bursts over subnormals, one sample at each end, streams
shorter than one filter half, and an odd stereo value count.  The rates are the standard ones, the limits 4 000 and 384 000,
31 250 with and without at_unity, its neighbours 31 249 and 31 251, and seeded draws in between.  The tables are the two
vendored ones, the library's default, the long table of the fixtures, and `big` (oracle/rsref.py big_table: 24 578
coefficients, past the 16 384 that fit in LDS).

check_all() runs the reference binaries of `make -C oracle rsref` in spawned CPU worker processes: dcs_rsref_{default,long,
big} (tests/golden/resample/rs_driver.c over the unmodified converter) for the floats, dcs_encrate_ref and its UBSan build
for the encoder cases, classified as tests/enc_cases.py does.  The restatement's result (tests/resample_ref.py, and
enc_ref / enc93_ref after it) comes with every short case.  At 31 250 Hz without at_unity the library passes the samples
through (its own rule; the reference runs the converter at ratio 1): there the expected floats are the downmix alone.  The
encoder cases all run with at_unity, as the reference encoder does."""
import collections
import concurrent.futures
import hashlib
import multiprocessing
import os
import subprocess
import tempfile

import numpy as np

import enc93_ref as E93
import enc_cases
import enc_ref as E
import resample_ref as R
from oracle import rsref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
MISSING = "oracle/_ref/dcs_rsref_* not built (needs /root/reference; `make -C oracle rsref`)"
MAX_WORKERS = 16            # the CPUs a GPU visit grants; never sized by os.cpu_count() alone

F32 = np.float32
TINY = float(np.finfo(F32).smallest_subnormal)          # 2^-149
NORM_MIN = float(np.finfo(F32).tiny)                    # 2^-126
FLT_MAX = float(np.finfo(F32).max)

TABLES = ("fastest", "medium", "default", "long", "big")
# table -> (binary, converter slot): the best-quality slot (0) holds the binary's own table
EXES = {"default": ("dcs_rsref_default", 0), "medium": ("dcs_rsref_default", 1), "fastest": ("dcs_rsref_default", 2),
        "long": ("dcs_rsref_long", 0), "big": ("dcs_rsref_big", 0)}
ENC_EXE, ENC_SAN = os.path.join(REF_DIR, "dcs_encrate_ref"), os.path.join(REF_DIR, "dcs_encrate_ref_san")

STANDARD = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000)
RATE_CLASSES = ("standard", "limit", "unity", "near_unity", "random")

Case = collections.namedtuple("Case", "name kind pcm rate channels table at_unity rate_class")
Result = collections.namedtuple("Result", "name table kind count sha256 ref want")
EncCase = collections.namedtuple("EncCase", "name kind pcm rate channels family version type subtype")
EncResult = collections.namedtuple("EncResult", "name family kind status kinds ref want")

_TABLES = {}


def tables():
    """{name: (float32 coefficients, increment)} from tests/golden/resample_filters.npz; big from the default one"""
    if not _TABLES:
        for k in ("fastest", "medium", "default", "long"):
            _TABLES[k] = rsref.npz_table(k)
        _TABLES["big"] = rsref.big_table(*_TABLES["default"])
    return _TABLES


def checker_available():
    return all(os.path.exists(os.path.join(REF_DIR, b)) for b in rsref.BINARIES)


# ----------------------------------------------------------------------------------------------------------- the signals

def _noise(rng, n):
    return rng.uniform(-1, 1, n).astype(F32)


def _subnormal(rng, n):
    """f32 subnormals only: every product with a coefficient, and every output, stays below 2^-126"""
    return (rng.integers(-(1 << 22), 1 << 22, n).astype(np.float64) * TINY).astype(F32)


def _neg_zero(rng, n):
    return np.full(n, -0.0, F32)


def _signed_zeros(rng, n):
    return np.where(rng.random(n) < 0.5, F32(-0.0), F32(0.0)).astype(F32)


def _tiny_normal(rng, n):
    """normals between 2^-126 and 2e-38: the outputs cross into the subnormal range"""
    return (rng.choice([-1.0, 1.0], n) * rng.uniform(NORM_MIN, 2e-38, n)).astype(F32)


def _decay(rng, n):
    """noise decaying from 1 to e^-100: through every f32 exponent down to the subnormals"""
    return (rng.uniform(-1, 1, n) * np.exp(-100.0 * np.arange(n) / max(n - 1, 1))).astype(F32)


def _huge(rng, n):
    """noise at 1e38, or at 3.3e38, where the sum of a few neighbours passes FLT_MAX and the cast to f32 gives +-inf"""
    return (rng.uniform(-1, 1, n) * rng.choice([1e38, 3.3e38])).astype(F32)


def _flt_max_alt(rng, n):
    """+-FLT_MAX alternating every 1, 2, 5 or 17 values: the f64 sums stay finite; where the filter passes the square its
    overshoot rounds to +-inf in the cast to f32"""
    half = int(rng.choice([1, 2, 5, 17]))
    return np.where((np.arange(n) // half) & 1, F32(-FLT_MAX), F32(FLT_MAX)).astype(F32)


def _spikes(rng, n):
    """3e38 spikes over 1e-30 noise, on even value indices only (a stereo pair then never holds two)"""
    x = (rng.uniform(-1, 1, n) * 1e-30).astype(F32)
    pos = 2 * rng.integers(0, (n + 1) // 2, max(1, n // 50))
    x[pos] = (rng.choice([-1.0, 1.0], len(pos)) * 3e38).astype(F32)
    return x


def _cancel(rng, n):
    """pairs a, -a at a scale of 1, 1e30 or 1e-30: neighbours cancel in the sums, a stereo pair downmixes to 0"""
    a = (rng.uniform(-1, 1, (n + 1) // 2) * rng.choice([1.0, 1e30, 1e-30])).astype(F32)
    x = np.empty(n, F32)
    x[0::2] = a
    x[1::2] = -a[:n // 2]
    return x


def _int16_grid(rng, n):
    return (rng.integers(-32768, 32768, n).astype(F32) / F32(32768)).astype(F32)


def _half_ulp(rng, n):
    vals = np.array([0.5, np.nextafter(F32(0.5), F32(1)), np.nextafter(F32(0.5), F32(0))], F32)
    return (vals[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], n).astype(F32)).astype(F32)


def _bursts(rng, n):
    """short loud bursts over a floor of subnormals"""
    x = _subnormal(rng, n)
    for _ in range(int(rng.integers(1, 4))):
        a = int(rng.integers(0, n))
        b = min(n, a + int(rng.integers(1, 60)))
        x[a:b] = (rng.uniform(-0.5, 0.5, b - a)).astype(F32)
    return x


def _ends(rng, n):
    """one nonzero sample at each end, silence between"""
    amps = [1.0, -1.0, TINY, -TINY, 0.5, NORM_MIN, 1e38, -FLT_MAX]
    x = np.zeros(n, F32)
    x[-1] = amps[rng.integers(len(amps))]
    x[0] = amps[rng.integers(len(amps))]
    return x


# (name, generator); "short" and "odd_stereo" are noise whose length and channel count _case() fixes
KINDS = [("subnormal", _subnormal), ("neg_zero", _neg_zero), ("signed_zeros", _signed_zeros), ("tiny_normal", _tiny_normal),
         ("decay", _decay), ("huge", _huge), ("flt_max_alt", _flt_max_alt), ("spikes", _spikes), ("cancel", _cancel),
         ("int16_grid", _int16_grid), ("half_ulp", _half_ulp), ("bursts", _bursts), ("ends", _ends), ("short", _noise),
         ("odd_stereo", _noise)]
KIND_NAMES = [k for k, _ in KINDS]


def _rate(rng, cls):
    if cls == "standard":
        return int(STANDARD[rng.integers(len(STANDARD))])
    if cls == "limit":
        return int((R.MIN_RATE, R.MAX_RATE)[rng.integers(2)])
    if cls == "unity":
        return 31250
    if cls == "near_unity":
        return int((31249, 31251)[rng.integers(2)])
    return int(rng.integers(R.MIN_RATE, R.MAX_RATE + 1))


def _case(rng, prefix, j, kind, fn, cls, table, at_unity):
    rate = _rate(rng, cls)
    ch = int(rng.integers(1, 3))
    n = int(rng.integers(1, 41)) if rng.random() < 0.35 else int(rng.integers(40, 1500 if table in ("long", "medium") else 3000))
    if kind == "short":             # fewer mono samples than half_filter_chan_len
        c, inc = tables()[table]
        n = int(rng.integers(1, max(2, min(R.params(len(c), inc, rate)[0], 40)))) * ch
    if kind == "odd_stereo":
        ch, n = 2, n | 1
    x = fn(rng, n)
    with np.errstate(over="ignore"):
        if not np.isfinite(R.downmix(x, ch)).all():     # a pair whose sum overflows: the library refuses it; the values as mono
            ch = 1
    assert x.dtype == F32 and np.isfinite(x).all()
    return Case("%s/%d/%s/%s/%d/%dch/%d" % (prefix, j, table, kind, rate, ch, n), kind, x, rate, ch, table, at_unity, cls)


def case_set(seed, k):
    """the k-th set of generator `seed`: one case of every kind on table TABLES[k % 5]; the flag alternates every five sets,
    the rate classes rotate through the kinds from set to set"""
    rng = np.random.default_rng([seed, k])
    table, at_unity = TABLES[k % len(TABLES)], (k // len(TABLES)) % 2 == 0
    return [_case(rng, "r%x-%d" % (seed, k), j, kind, fn, RATE_CLASSES[(j + k // len(TABLES)) % len(RATE_CLASSES)], table, at_unity)
            for j, (kind, fn) in enumerate(KINDS)]


# streams of 1 to 3 values the GPU test interleaves with a set's cases, so a call's stream count can be made anything
FILLS = [(np.zeros(1, F32), 44100, 1), (np.array([1.0, -1.0, TINY], F32), 4000, 2), (np.array([-1.0, 0.5], F32), 31250, 1),
         (np.array([TINY, -0.0, 0.25], F32), 8000, 1)]


def fillers(seed, k):
    table, at_unity = TABLES[k % len(TABLES)], (k // len(TABLES)) % 2 == 0
    return [Case("fill%x-%d/%d/%s" % (seed, k, j, table), "filler", x, rate, ch, table, at_unity, "filler")
            for j, (x, rate, ch) in enumerate(FILLS)]


# (table, channels, fewest values, most values): long streams at random rates; count and sha256 only.  The stereo one holds
# more than 2 x 262 144 values, an odd number of them.
LONG = [("default", 1, 200000, 400000), ("default", 2, 2 * 262144 + 1, 2 * 262144 + 60001), ("long", 1, 150000, 250000),
        ("big", 1, 200000, 300000), ("fastest", 1, 200000, 400000), ("medium", 2, 150001, 250001)]


def long_case(seed, i):
    rng = np.random.default_rng([seed, 0x10E6, i])
    table, ch, lo, hi = LONG[i]
    n = int(rng.integers(lo, hi))
    n = n | 1 if ch == 2 else n
    rate = _rate(rng, "random")
    x = R.lcg_signal(seed + i, n, 0.5)
    return Case("long%x-%d/%s/lcg/%d/%dch/%d" % (seed, i, table, rate, ch, n), "long", x, rate, ch, table, True, "random")


def many_pool(seed, size=50):
    """`size` distinct short quiet streams of mixed rates and channel counts on the default table, without at_unity: what one
    call of more than 65 535 streams is drawn from.  Each resamples to at least one sample and stays far inside [-1, 1], so
    the encoder takes it too."""
    rng = np.random.default_rng([seed, 0x3A27])
    c, inc = tables()["default"]
    quiet = [("subnormal", _subnormal), ("neg_zero", _neg_zero), ("tiny_normal", _tiny_normal),
             ("decay", lambda r, n: _decay(r, n) * F32(0.5)), ("int16_grid", lambda r, n: _int16_grid(r, n) * F32(0.25)),
             ("bursts", _bursts), ("half_ulp", _half_ulp)]
    out = []
    for j in range(size):
        kind, fn = quiet[j % len(quiet)]
        rate = _rate(rng, RATE_CLASSES[j % len(RATE_CLASSES)])
        ch = int(rng.integers(1, 3))
        n = max(1, int(rng.integers(1, 300) * rate / 31250.0))
        while R.count(n * ch, rate, len(c), inc, ch, R.AT_UNITY) < 1:
            n += 1 + n // 4
        n = n * ch - (1 if ch == 2 and j % 4 == 1 else 0)
        out.append(Case("many%x/%d/%s/%d/%dch/%d" % (seed, j, kind, rate, ch, n), kind, fn(rng, n).astype(F32), rate, ch, "default",
                        False, RATE_CLASSES[j % len(RATE_CLASSES)]))
    return out


def peak_cases(seed):
    """default table, never at 31 250 Hz: streams whose resampled peak is a subnormal, slightly above or below 1, far above
    it, or infinite -- for the encoder's refusal, which must follow the reference's floats (all but the ladder at 44 100 Hz
    rotate through six rates)"""
    rng = np.random.default_rng([seed, 0x9EA4])
    one_up, one_down = float(np.nextafter(F32(1), F32(2))), float(np.nextafter(F32(1), F32(0)))
    n = 1200
    sq = np.where((np.arange(n) // 50) & 1, 1.0, -1.0)
    sig = [("dc_one", np.full(n, 1.0)), ("dc_below_one", np.full(n, one_down)), ("dc_minus_one", np.full(n, -1.0)),
           ("dc_0.9999", np.full(n, 0.9999)), ("dc_0.99", np.full(n, 0.99)), ("square_1", sq), ("square_0.5", 0.5 * sq),
           ("decay_1", _decay(rng, n)), ("decay_0.5", _decay(rng, n) * F32(0.5)), ("subnormal", _subnormal(rng, n)),
           ("tiny", np.full(n, TINY)), ("flt_max_alt", _flt_max_alt(rng, n)), ("huge", _noise(rng, n) * F32(1e38)),
           ("ends_max", _ends(rng, n)), ("dc_one_up_in", np.full(n, one_up)), ("noise_1", _noise(rng, n)),
           ("dc_flt_max", np.full(n, FLT_MAX)), ("noise_3e38", _noise(rng, n) * F32(3e38))]
    # the filter's step response overshoots a DC level by about a tenth: a ladder of levels whose peaks straddle 1
    sig += [("dc_%.4f" % a, np.full(n, a)) for a in np.arange(0.8950, 0.9151, 0.0025)]
    rates = (44100, 48000, 22050, 31251, 4000, 96000)
    rate_of = lambda j, kind: 44100 if kind.startswith("dc_0.") and len(kind) == 9 else rates[j % len(rates)]
    return [Case("peak%x/%d/%s/%d" % (seed, j, kind, rate_of(j, kind)), kind, np.asarray(x).astype(F32), rate_of(j, kind), 1,
                 "default", False, "peak") for j, (kind, x) in enumerate(sig)]


# ------------------------------------------------------------------------------------------------------ the encoder half

ENC_FAMILIES = {"94": (0x9400, -1, -1), "93b": (0x9302, -1, -1), "93a": (0x9301, 0, -1)}
ENC_RATES = (4000, 22050, 31250, 44100, 48000, 384000, "random", 31249)


def _music(rng, n, rate):
    t = np.arange(n) / float(rate)
    f0 = rng.uniform(60, 900)
    x = sum(rng.uniform(0.05, 0.3) / h * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6)) for h in range(1, 5))
    return (x * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) * 0.5 + rng.normal(0, 0.01, n)).astype(F32)


# kinds whose resampled peak stays inside [-1, 1] (the library refuses the others)
ENC_KINDS = [("subnormal", lambda r, n, rate: _subnormal(r, n)), ("neg_zero", lambda r, n, rate: _neg_zero(r, n)),
             ("tiny_normal", lambda r, n, rate: _tiny_normal(r, n)), ("decay", lambda r, n, rate: _decay(r, n) * F32(0.5)),
             ("int16_grid", lambda r, n, rate: _int16_grid(r, n) * F32(0.25)), ("bursts", lambda r, n, rate: _bursts(r, n)),
             ("music", _music)]


def enc_set(seed, k):
    """the k-th encoder set: one case of every encoder kind for family k % 3 (one dcs_encode_streams_at call)"""
    rng = np.random.default_rng([seed, 0xE2C0, k])
    fam = list(ENC_FAMILIES)[k % 3]
    version, typ, sub = ENC_FAMILIES[fam]
    out = []
    for j, (kind, fn) in enumerate(ENC_KINDS):
        rate = ENC_RATES[(j + k // 3) % len(ENC_RATES)]
        rate = _rate(rng, "random") if rate == "random" else rate
        ch = int(rng.integers(1, 3))
        n = max(40, int(rng.integers(250, 5000) * rate / 31250.0)) * ch - int(ch == 2 and rng.random() < 0.5)
        x = fn(rng, n, rate).astype(F32)
        out.append(EncCase("e%x-%d/%d/%s/%s/%d/%dch/%d" % (seed, k, j, fam, kind, rate, ch, n), kind, x, rate, ch, fam, version, typ, sub))
    return out


# ---------------------------------------------------------------------------------------------------------- the checker

def _run(argv):
    r = subprocess.run(argv, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("%s exited %d: %s" % (" ".join(argv[:1] + argv[3:]), r.returncode, r.stderr[-2000:]))
    return r.stderr


def reference_floats(x, rate, channels, table, tmp):
    """libsamplerate's output, as bytes, for the values x run as the reference encoder runs the converter"""
    exe, conv = EXES[table]
    src, dst = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.f32")
    np.asarray(x, "<f4").tofile(src)
    _run([os.path.join(REF_DIR, exe), src, dst, str(conv), str(rate), str(channels)])
    with open(dst, "rb") as f:
        return f.read()


def check(case, with_reference=True):
    """-> Result: ref = the reference's floats (None at the pass-through, without a checker, and for a long case, which
    keeps count and sha256 alone); want = the restatement's floats (None for a long case)"""
    c, inc = tables()[case.table]
    flags = R.AT_UNITY if case.at_unity else 0
    want = None if case.kind == "long" else R.resample(case.pcm, case.rate, c, inc, case.channels, flags)
    ref = count = sha = None
    if R.pass_through(case.rate, flags):
        ref = None
    elif with_reference:
        with tempfile.TemporaryDirectory() as tmp:
            raw = reference_floats(case.pcm, case.rate, case.channels, case.table, tmp)
        count, sha = len(raw) // 4, hashlib.sha256(raw).hexdigest()
        ref = None if case.kind == "long" else np.frombuffer(raw, "<f4").copy()
    if count is None and want is not None:
        count, sha = len(want), digest(want)
    return Result(case.name, case.table, case.kind, count, sha, ref, want)


def digest(y):
    return hashlib.sha256(np.asarray(y, "<f4").tobytes()).hexdigest()


def same_bits(a, b):
    return len(a) == len(b) and np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def _run_encoder(exe, case, tmp):
    src, dst = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.bin")
    np.asarray(case.pcm, "<f4").tofile(src)
    report = _run([exe, src, dst, str(case.rate), str(case.channels), "%x" % case.version, str(case.type), str(case.subtype)])
    with open(dst, "rb") as f:
        return f.read(), report


def restate_encoder(case):
    """enc_ref / enc93_ref after resample_ref (the converter runs at 31 250 Hz too) -> (bytes, times the Keep +15 rule fired)"""
    c, inc = tables()["default"]
    y = R.resample(case.pcm, case.rate, c, inc, case.channels, R.AT_UNITY)
    if case.family == "94":
        return E.encode(y, (case.type, case.subtype))[0], 0
    s, _, _, fired = E93.encode(y, case.version, case.type)
    return s, fired


def check_encoder(case, with_reference=True):
    """as enc_cases.check: "kept" (the reference's bytes are the contract), "rule" (kept, but the OS93 Keep +15 rule fired:
    the library's bytes), "dropped" (a bounds or float-cast report), "unchecked" (no checker)"""
    want, fired = restate_encoder(case)
    kinds, ref, status = [], None, "unchecked"
    if with_reference:
        with tempfile.TemporaryDirectory() as tmp:
            _, report = _run_encoder(ENC_SAN, case, tmp)
            kinds = enc_cases.ubsan_kinds(report)
            if any(k != "shift" for k in kinds):
                status = "dropped"
            else:
                ref, _ = _run_encoder(ENC_EXE, case, tmp)
                status = "rule" if fired else "kept"
    return EncResult(case.name, case.family, case.kind, status, kinds, ref, want)


COUNT_GROUP = 8


def count_draws(seed, i):
    """the i-th group of (values, rate, channels, table) draws for the count alone: lengths log-uniform up to 2 000 000"""
    rng = np.random.default_rng([seed, 0xC027, i])
    out = []
    for j in range(COUNT_GROUP):
        table = TABLES[(i + j) % len(TABLES)]
        top = 2000000 if table != "long" else 500000
        n = int(np.exp(rng.uniform(0, np.log(top))))
        ch = int(rng.integers(1, 3))
        cls = RATE_CLASSES[int(rng.integers(len(RATE_CLASSES)))]
        out.append((max(1, n), _rate(rng, cls), ch, table))
    return out


def _reference_count(n, rate, ch, table):
    with tempfile.TemporaryDirectory() as tmp:
        return len(reference_floats(np.zeros(n, F32), rate, ch, table, tmp)) // 4


def keys(seed, n_sets=0, n_enc_sets=0, n_counts=0, with_fillers=False, with_long=False, with_many=False, with_peak=False):
    """the work items of a run, the slowest first"""
    out = [("count", seed, i) for i in range(n_counts)]
    out += [("long", seed, i) for i in range(len(LONG))] if with_long else []
    out += [("enc", seed, k) for k in range(n_enc_sets)]
    out += [(kind, seed, k) for k in range(n_sets) for kind in (("set", "fill") if with_fillers else ("set",))]
    out += [("many", seed)] if with_many else []
    out += [("peak", seed)] if with_peak else []
    return out


def cases_of(key):
    kind = key[0]
    if kind == "set":
        return case_set(key[1], key[2])
    if kind == "fill":
        return fillers(key[1], key[2])
    if kind == "long":
        return [long_case(key[1], key[2])]
    if kind == "many":
        return many_pool(key[1])
    if kind == "peak":
        return peak_cases(key[1])
    if kind == "enc":
        return enc_set(key[1], key[2])
    raise KeyError(key)


def _check_key(key, with_reference):
    if key[0] == "count":
        return [(d, _reference_count(*d) if with_reference else None) for d in count_draws(key[1], key[2])]
    if key[0] == "enc":
        return [check_encoder(c, with_reference) for c in cases_of(key)]
    res = [check(c, with_reference) for c in cases_of(key)]
    if key[0] == "many":            # the pool feeds the encoder as well
        res += [check_encoder(EncCase(c.name + "/enc", c.kind, c.pcm, c.rate, c.channels, "94", 0x9400, -1, -1), with_reference)
                for c in cases_of(key)]
    return res


def check_all(work, with_reference=True, workers=None):
    """check every case of the work items in fresh worker processes (spawned, CPU only: they never open the GPU), at most
    MAX_WORKERS of them -> {case name: Result or EncResult}, and {"counts": [((values, rate, channels, table), count)]}"""
    workers = workers or max(1, min(MAX_WORKERS, os.cpu_count() or 1, len(work) or 1))
    out = {"counts": []}
    ctx = multiprocessing.get_context("spawn")
    with concurrent.futures.ProcessPoolExecutor(workers, mp_context=ctx) as pool:
        for key, res in zip(work, pool.map(_check_key, work, [with_reference] * len(work))):
            if key[0] == "count":
                out["counts"] += res
            else:
                for r in res:
                    out[r.name] = r
    return out


def format_matches(rows):
    """rows: (table, kind) per matched case -> a table x kind tally"""
    t = collections.Counter(rows)
    kinds = sorted({k for _, k in t})
    lines = ["%-8s" % "table" + "".join(" %5s" % k[:5] for k in kinds) + "  total"]
    for tab in sorted({a for a, _ in t}):
        lines.append("%-8s" % tab + "".join(" %5d" % t[tab, k] for k in kinds) + " %6d" % sum(t[tab, k] for k in kinds))
    return "\n".join(lines)


def enc_tally(results):
    out = {fam: collections.Counter() for fam in ENC_FAMILIES}
    for r in results:
        out[r.family][r.status] += 1
    return out


def format_enc_tally(t):
    return "\n".join("%-4s kept %4d  rule %3d  dropped %3d" % (f, c["kept"], c["rule"], c["dropped"]) for f, c in t.items())
