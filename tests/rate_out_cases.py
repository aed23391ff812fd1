"""Seeded adversarial cases for the output-rate converter (dcs_resample_out_streams, dcs_decode_streams_at,
dcs_decode_streams_flac_at), and the compiled libsamplerate as their checker (test infrastructure).  Recipes only; no
samples are committed.

A case is one int16 stream at 31 250 Hz with its table and output rate.  The cases of one (table, rate) are one call, so
that every length reads the record table the call's longest stream walked (rsOutWalks, dcs_resample.hip.h) and the host
pool has many distinct lengths to count.

  Rates     every rate in 4000 .. 65535 for which 31250 / rate is a dyadic rational (dyadic_rates(): the 28 rates 5^b 2^a in
            range), where the walk's input_index is exact and lands on .5 in fmod_one and on the end rule's boundary
            (at .5 either tie rule of rint leaves fmod_one the same remainder; it is the end rule that tells: written with
            >= it changes counts at 11 of these rates, the multiples of 5^4, and at no other rate of the list); the
            neighbours 31249 31251 4001 65534 62499 62501; 11025 22050 44100 48000; seeded draws.  31 250 runs with at_unity
            (the binary always runs the converter).  The full list runs on the default table; the other tables take the
            dyadic and the common rates and 10 draws of their own.
  Lengths   NAMED; b_len - 1, b_len, b_len + 1 and 2 b_len + 333 with b_len the converter's ring (not on the long table,
            whose ring is 256 000 samples); 30 seeded lengths up to 9000; on LONG_RATES one stream more whose walk makes more
            than 65 536 outputs, which sends the table's walk to the host (rsHostRoute).
  Content   full-scale LCG noise; the +-32767 square (the clip case); noise of +-1 .. +-3 LSB, where |y| < 2^-8 and the lrint
            and the flooring shift of src_float_to_short_array meet fractions and ties; an impulse at sample 0 and one at
            sample n - 1; DC at both signs; silence.  The kinds rotate over a call's streams and from call to call.

calls(table, rate) gives the lists a test runs for one (table, rate): the full list, and where that list's table is walked
on the host also the list without the streams that put it there, which a device lane walks.

THINNING.  The numpy restatement (tests/decode_rate_ref.py) converts a stream of more than RESTATE_MAX samples only in every
RESTATE_EVERY-th rate of its table's list (restated()).  That bounds the time of the one comparison restatement == binary;
the count, the walk records and the GPU take every case.

check_all() runs oracle/_ref/dcs_rsout_{default,long,big} (tests/golden/resample/out_rate_driver.c over the unmodified
converter, `make -C oracle rsref`) in spawned CPU worker processes."""
import collections
import concurrent.futures
import functools
import hashlib
import multiprocessing
import os
import subprocess
import tempfile

import numpy as np

import decode_rate_ref as Q
import resample_ref as R
from oracle import rsref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
MISSING = "oracle/_ref/dcs_rsout_* not built (needs /root/reference; `make -C oracle rsref`)"
MAX_WORKERS = 16            # the CPUs a GPU visit grants; never sized by os.cpu_count() alone
SEED = 0x0A7E5

TABLES = ("default", "medium", "fastest", "long", "big")
# table -> (binary, converter slot): the best-quality slot (0) holds the binary's own table
EXES = {"default": ("dcs_rsout_default", 0), "medium": ("dcs_rsout_default", 1), "fastest": ("dcs_rsout_default", 2),
        "long": ("dcs_rsout_long", 0), "big": ("dcs_rsout_big", 0)}
IN_RATE = 31250
NEIGHBOURS = (31249, 31251, 4001, 65534, 62499, 62501)
COMMON = (11025, 22050, 44100, 48000)
N_RANDOM_RATES = {"default": 40, "medium": 10, "fastest": 10, "long": 10, "big": 10}
NAMED = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 97, 239, 240, 241, 4095, 4096, 4097)
N_RANDOM_LENGTHS = 30
MAX_RANDOM_LENGTH = 9000
# the rates at which a call gains one stream whose walk makes more than HOST_WALK_MIN outputs (at the higher rates of the
# tables with a ring of 30 720 samples 2 b_len + 333 does that by itself)
LONG_RATES = {"default": (8000, 22050, 31250, 31251), "medium": (31250,), "fastest": (16000, 31250), "long": (31250, 48000),
              "big": (16000, 31250)}
HOST_WALK_MIN = 65536       # kRsHostWalkMin
LDS_MAX_COEFFS = 16384      # kRsLdsMaxCoeffs
KINDS = ("noise", "square", "lsb", "impulse0", "impulseN", "dc+", "dc-", "silence")
RESTATE_MAX = 4097
RESTATE_EVERY = 6

Case = collections.namedtuple("Case", "name table rate n kind seed")
# out: the binary's int16 samples; hi, lo: how many outputs its two clamping branches took; peak: the bits of the largest |y|
# of its float output; want, want_info: the restatement's samples and info (None where thinned); walk: (count, sha256) of
# the restatement's walk records (None where not asked for)
Result = collections.namedtuple("Result", "name out hi lo peak want want_info walk")

_TABLES = {}


def tables():
    """{name: (float32 coefficients, increment)}: default, medium and fastest from tests/golden/resample_filters.npz, long
    from tests/golden/decode_rate_golden.npz, big from the default one"""
    if not _TABLES:
        for k in ("default", "medium", "fastest"):
            _TABLES[k] = rsref.npz_table(k)
        _TABLES["long"] = rsref.out_long_table()
        _TABLES["big"] = rsref.big_table(*_TABLES["default"])
    return _TABLES


def checker_available():
    return all(os.path.exists(os.path.join(REF_DIR, exe)) for exe, _ in EXES.values())


def buffer_len(table):
    c, inc = tables()[table]
    return R.buffer_len(len(c), inc)


# ----------------------------------------------------------------------------------------------------- rates and lengths

@functools.lru_cache(maxsize=None)
def dyadic_rates():
    """every rate in range with 31250 / rate = k / 2^m: 31250 = 2 x 5^6, so the rate's odd part divides 5^6"""
    out = [r for r in range(Q.MIN_RATE, Q.MAX_RATE + 1) if 5 ** 6 % (r // (r & -r)) == 0]
    assert len(out) == 28 and all((IN_RATE << 16) % r == 0 for r in out) and {4000, 4096, 15625, 31250, 64000} <= set(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rates(table):
    """the table's rate list; a rate's index in it sets the rotation of kinds and the thinning"""
    named = list(dyadic_rates()) + (list(NEIGHBOURS) if table == "default" else []) + list(COMMON)
    rng = np.random.default_rng([SEED, 1, TABLES.index(table)])
    drawn = []
    while len(drawn) < N_RANDOM_RATES[table]:
        r = int(rng.integers(Q.MIN_RATE, Q.MAX_RATE + 1))
        if r not in named and r not in drawn:
            drawn.append(r)
    return tuple(named + drawn)


def long_length(rate):
    """a length whose estimate nIn / step + 4 is well past HOST_WALK_MIN"""
    return int(np.ceil((HOST_WALK_MIN + 600) * float(IN_RATE) / rate))


@functools.lru_cache(maxsize=None)
def lengths(table, rate):
    out = list(NAMED)
    if table != "long":
        b = buffer_len(table)
        out += [b - 1, b, b + 1, 2 * b + 333]
    rng = np.random.default_rng([SEED, 2, TABLES.index(table), rate])
    n_named = len(out)
    while len(out) < n_named + N_RANDOM_LENGTHS:
        n = int(rng.integers(1, MAX_RANDOM_LENGTH + 1))
        if n not in out:
            out.append(n)
    if rate in LONG_RATES[table]:
        out.append(long_length(rate))
    assert len(set(out)) == len(out)
    return tuple(sorted(out))


def slots(n, rate):
    """rsSlots: the estimate rsHostRoute decides by, (uint64)((double)nIn / step) + 4 with step = 1 / (rate / 31250.0)"""
    return int(float(n) / (1.0 / (float(rate) / float(IN_RATE)))) + 4


def host_walked(ns, rate):
    """rsOutWalks walks the table, the longest stream's records, on the host where that stream as a list of its own is
    routed there: more than HOST_WALK_MIN estimated outputs (it is then all of its list, so the share rule holds)"""
    return slots(max(ns), rate) > HOST_WALK_MIN


# --------------------------------------------------------------------------------------------------------------- content

_LCG_BLOCK = 4096


@functools.lru_cache(maxsize=None)
def _lcg_jumps():
    a, c = np.empty(_LCG_BLOCK, np.uint64), np.empty(_LCG_BLOCK, np.uint64)
    a[0], c[0] = 1664525, 1013904223
    for k in range(1, _LCG_BLOCK):
        a[k] = (a[k - 1] * np.uint64(1664525)) & np.uint64(0xFFFFFFFF)
        c[k] = (c[k - 1] * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)
    return a, c


def lcg(seed, n):
    """n values of x' = (1664525 x + 1013904223) mod 2^32 from `seed` (decode_rate_ref.lcg16's generator, in blocks)"""
    a, c = _lcg_jumps()
    x = np.empty(n, np.uint64)
    v = np.uint64(seed & 0xFFFFFFFF)
    for i in range(0, n, _LCG_BLOCK):
        m = min(_LCG_BLOCK, n - i)
        x[i:i + m] = (a[:m] * v + c[:m]) & np.uint64(0xFFFFFFFF)
        v = x[i + m - 1]
    return x.astype(np.int64)


def make(case):
    """the case's int16 samples"""
    n, kind = case.n, case.kind
    if kind == "noise":
        return ((lcg(case.seed, n) >> 16) - 32768).astype(np.int16)
    if kind == "square":            # +-32767, period 100 samples, the phase by the seed: short streams see both signs too
        return np.where(((np.arange(n) + 25 * (case.seed % 4)) // 50) & 1, -32767, 32767).astype(np.int16)
    if kind == "lsb":
        a = 1 + case.seed % 3
        return ((lcg(case.seed, n) >> 16) % (2 * a + 1) - a).astype(np.int16)
    x = np.zeros(n, np.int16)
    if kind == "impulse0":
        x[0] = (32767, -32768, 1, -1)[case.seed % 4]
    elif kind == "impulseN":
        x[-1] = (32767, -32768, 1, -1)[case.seed % 4]
    elif kind == "dc+":
        x[:] = 32767
    elif kind == "dc-":
        x[:] = -32768 if case.seed % 2 else -32767
    else:
        assert kind == "silence"
    return x


@functools.lru_cache(maxsize=None)
def call_cases(table, rate):
    """the full list of (table, rate), by rising length"""
    i, t = rates(table).index(rate), TABLES.index(table)
    out = []
    for j, n in enumerate(lengths(table, rate)):
        kind = KINDS[(j + 3 * i + t) % len(KINDS)]
        out.append(Case("%s/%d/%d/%s" % (table, rate, n, kind), table, rate, n, kind, 1 + 7 * n + 31 * i + t))
    return tuple(out)


def calls(table, rate):
    """[(what, cases)]: the full list and, where its table is walked on the host, the rest as a call of its own"""
    full = call_cases(table, rate)
    out = [("full", full)]
    if host_walked([c.n for c in full], rate):
        rest = tuple(c for c in full if slots(c.n, rate) <= HOST_WALK_MIN)
        assert not host_walked([c.n for c in rest], rate)
        out.append(("device-walked rest", rest))
    return out


def keys():
    return [(t, r) for t in TABLES for r in rates(t)]


def restated(case):
    """the thinning rule (see the module's text)"""
    return case.n <= RESTATE_MAX or rates(case.table).index(case.rate) % RESTATE_EVERY == 0


# ----------------------------------------------------------------------------------------------------------- the checker

def reference_convert(pcm, table, rate, tmp):
    """the driver on int16 samples -> (libsamplerate's int16 output, its float32 output)"""
    exe, conv = EXES[table]
    src, dst, dstf = os.path.join(tmp, "in.s16"), os.path.join(tmp, "out.s16"), os.path.join(tmp, "out.f32")
    np.asarray(pcm, "<i2").tofile(src)
    r = subprocess.run([os.path.join(REF_DIR, exe), src, dst, dstf, str(conv), str(rate)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("%s %d %d exited %d: %s" % (exe, conv, rate, r.returncode, r.stderr[-2000:]))
    return np.fromfile(dst, "<i2"), np.fromfile(dstf, "<f4")


def clamp_counts(yf):
    """how many outputs each clamping branch of src_float_to_short_array takes on the floats yf"""
    v = np.asarray(yf, np.float32).astype(np.float64) * 2147483648.0
    return int((v >= 2147483647.0).sum()), int((v <= -2147483648.0).sum())


def peak_bits(yf):
    return int((np.float32(np.max(np.abs(yf))) if len(yf) else np.float32(0)).view(np.uint32))


def walk_digest(pos, sfi):
    return len(pos), hashlib.sha256(np.asarray(pos, "<i8").tobytes() + np.asarray(sfi, "<i4").tobytes()).hexdigest()


def check_call(key, with_reference=True, with_restatement=False, with_walks=False):
    """every case of the call `key` -> [Result]"""
    table, rate = key
    c, inc = tables()[table]
    cases = call_cases(table, rate)
    mine = [case for case in cases if with_restatement and restated(case)]
    floats = dict(zip(mine, Q.convert_float_many([make(case) for case in mine], rate, c, inc))) if mine else {}
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for case in cases:
            y = hi = lo = peak = want = want_info = walk = None
            if with_reference:
                y, yf = reference_convert(make(case), table, rate, tmp)
                (hi, lo), peak = clamp_counts(yf), peak_bits(yf)
            if case in floats:
                want, clipped = Q.float_to_short(floats[case])
                want_hi, want_lo = clamp_counts(floats[case])
                assert clipped == want_hi + want_lo
                want_info = dict(nOut=len(want), hi=want_hi, lo=want_lo, peak=peak_bits(floats[case]))
            if with_walks:
                walk = walk_digest(*Q.walk(case.n, len(c), inc, rate))
            out.append(Result(case.name, y, hi, lo, peak, want, want_info, walk))
    return out


def check_all(work, with_reference=True, with_restatement=False, with_walks=False, workers=None):
    """check_call on every key of `work` in fresh worker processes (spawned, CPU only: they never open the GPU), at most
    MAX_WORKERS of them -> {case name: Result}"""
    workers = workers or max(1, min(MAX_WORKERS, os.cpu_count() or 1, len(work) or 1))
    # the longest calls first: the low rates of the long table and the calls with a long stream
    order = sorted(work, key=lambda k: -sum(c.n for c in call_cases(*k)) * (4 if k[0] == "long" and with_restatement else 1))
    out = {}
    ctx = multiprocessing.get_context("spawn")
    with concurrent.futures.ProcessPoolExecutor(workers, mp_context=ctx) as pool:
        n = len(order)
        for res in pool.map(check_call, order, [with_reference] * n, [with_restatement] * n, [with_walks] * n):
            for r in res:
                out[r.name] = r
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """the binaries' output of every case, taken once per session and left unchanged"""
    return check_all(keys())


def clip_condition(results):
    """On the reference's output alone: at every rate >= 32000 of every table the square streams of the call take both
    clamping branches at least once.  -> the (table, rate) that miss it"""
    bad = []
    for table, rate in keys():
        if rate < 32000:
            continue
        sq = [results[c.name] for c in call_cases(table, rate) if c.kind == "square"]
        if not (sum(r.hi for r in sq) > 0 and sum(r.lo for r in sq) > 0):
            bad.append((table, rate))
    return bad
