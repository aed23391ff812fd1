"""Seeded adversarial encoder cases, and the compiled reference encoder as their checker (test infrastructure).

A case is one PCM stream with the family, layout and CompressionParams it is encoded with.  Cases come in sets that share
family, layout and params, so a set is one encoder call.  Everything is a pure function of (seed, set index): a worker
process rebuilds a set from its key instead of receiving the samples.

The signals aim at where a float kernel parts from x86-64 SSE and where the encoder's integer rules turn: f32 denormals
and band powers that underflow (powerNorm = 1/total becomes inf, or total == 0), -0.0 beside +0.0, exactly +-1.0 and
1 - 2^-24, int16 -32768 and 32767, single-sample impulses on frame edges, Nyquist-rate and full-scale squares -- and
music-like signals, so the searches have work.  The params include powerBandCutoff <= 0, == 1 and > 1, rates from 1 bit/s
(every band at 0 bits) to 10^8 (bitsPerBand > 31: the masked shift), a dynamic range or quantisation error of 0, and
negative values: everything paramsValid accepts.

check() runs the reference encoder (oracle/_ref/dcs_encref, built by `make -C oracle encref`) on a case, first its UBSan
build (dcs_encref_san), and classifies the case as the golden generators do: a bounds or float-cast report DROPS it (the
reference's bytes then depend on its binary layout); a shift report alone keeps it (the library's masked-shift rule,
INTEGRATION.md "Encoding").  A kept OS93 case in which the library's Keep +15 rule fired is a RULE case: its bytes are the
library's, not the reference's.  The restatement's result (tests/enc_ref.py, tests/enc93_ref.py) comes with it.

Layout `93a/T1`, the pair-table layout the reference cannot write, is not among FAMILIES: its seeded cases are
tests/enc93a_fuzz_cases.py, which takes the signal kinds from here and has the reference DECODER as its checker."""
import collections
import concurrent.futures
import multiprocessing
import os
import subprocess
import tempfile

import numpy as np

import enc_ref as E
import enc93_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "_ref", "dcs_encref")
SAN = os.path.join(ROOT, "oracle", "_ref", "dcs_encref_san")
MISSING = "oracle/_ref/dcs_encref not built (needs /root/reference; `make -C oracle encref`)"

F32 = np.float32
TINY = float(np.finfo(F32).smallest_subnormal)          # 2^-149
NORM_MIN = float(np.finfo(F32).tiny)                    # 2^-126
BELOW_ONE = float(np.nextafter(F32(1), F32(0)))          # 1 - 2^-24

# family -> (formatVersion, {layout: (streamFormatType, streamFormatSubType)}); OS93 has no sub-types (-1 is passed)
FAMILIES = {
    "94": (0x9400, {"wild": (-1, -1), "T0s0": (0, 0), "T0s3": (0, 3), "T1s0": (1, 0), "T1s3": (1, 3)}),
    "93b": (0x9302, {"wild": (-1, -1), "T0": (0, -1), "T1": (1, -1)}),
    "93a": (0x9301, {"wild": (-1, -1), "T0": (0, -1)}),
}
LAYOUTS = [(fam, lay) for fam, (_, lays) in FAMILIES.items() for lay in lays]
LONGEST = 65535 * 240                                   # samples in the longest stream the formats allow

Case = collections.namedtuple("Case", "name pcm family layout version type subtype params")

CUTOFFS = [0.0, -0.0, 1.0, float(np.nextafter(F32(1), F32(2))), BELOW_ONE, 1.5, 3.0, -0.5, -1e30, 1e30, 1e-30, 0.5, 0.8, 0.97,
           0.999]
RATES = [1, 7, 100, 1000, 2000, 4000, 8000, 16000, 24000, 64000, 128000, 320000, 1000000, 2000000, 10000000, 100000000]
MIN_DR = [0.0, -0.0, TINY, 1e-40, 1 / 32768, 10 / 32768, 40 / 32768, 0.01, 0.5, 1.0, 2.0, -1 / 32768]
MAX_QE = [0.0, TINY, 1e-40, 1 / 32768, 3 / 32768, 10 / 32768, 30 / 32768, 0.01, 0.5, 2.0, -10 / 32768]
LENGTHS = [1, 2, 239, 240, 241, 16 * 240 - 1, 16 * 240, 16 * 240 + 1, 479, 481]
# the frame k = x[240k - 16 .. 240k + 240): positions at the overlap's and the frame's edges
EDGES = [0, 1, 15, 16, 17, 223, 224, 225, 238, 239, 240, 241, 255, 256, 257, 463, 464, 479, 480]


def _params(rng):
    """each field the reference's default or, half the time, one of its edges; all exactly binary32"""
    p = dict(E.DEFAULTS)
    for key, edges in (("powerBandCutoff", CUTOFFS), ("targetBitRate", RATES), ("minimumDynamicRange", MIN_DR),
                       ("maximumQuantizationError", MAX_QE)):
        if rng.random() < 0.5:
            p[key] = edges[rng.integers(len(edges))]
    return {k: int(v) if k == "targetBitRate" else float(F32(v)) for k, v in p.items()}


def _length(rng):
    u = rng.random()
    if u < 0.6:
        return int(LENGTHS[rng.integers(len(LENGTHS))])
    if u < 0.97:
        return int(rng.integers(1, 240 * 64))
    return int(rng.integers(240 * 1000, 240 * 2500))      # a few long streams


def _music(rng, n):
    t = np.arange(n) / 31250.0
    f0 = rng.uniform(40, 2000)
    x = sum(rng.uniform(0, 0.5) / h * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6)) for h in range(1, int(rng.integers(2, 12))))
    x = x * (0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(0.5, 8) * t)) + rng.normal(0, rng.uniform(1e-4, 0.1), n)
    return np.clip(x * 10 ** rng.uniform(-3, 0.3), -1, 1)


def _denormal(rng, n):
    """f32 subnormals only (and zeros): every band power underflows to 0 or to a subnormal"""
    k = rng.integers(-(1 << int(rng.integers(1, 23))), 1 << int(rng.integers(1, 23)), n)
    x = (k.astype(np.float64) * TINY).astype(F32)
    x[rng.random(n) < rng.uniform(0, 0.5)] = 0
    return x


def _underflow(rng, n):
    """normal samples so small their squares are subnormal or zero; the band powers and their total underflow"""
    return (rng.normal(0, 1, n) * 10 ** rng.uniform(-44, -17)).astype(F32)


def _signed_zero(rng, n):
    x = np.where(rng.random(n) < rng.uniform(0, 1), F32(-0.0), F32(0.0)).astype(F32)
    if rng.random() < 0.4:
        x[rng.integers(n)] = F32(rng.choice([TINY, -TINY, NORM_MIN, -1.0]))
    return x


def _unit(rng, n):
    """+-1.0, +-(1 - 2^-24) and 0.5 steps: at and next to full scale"""
    vals = np.array([1.0, -1.0, BELOW_ONE, -BELOW_ONE, 0.5, -0.5, 0.0], F32)
    if rng.random() < 0.5:
        return vals[rng.integers(0, len(vals), n)]
    a = vals[rng.integers(0, 4)]
    return np.full(n, a, F32) if rng.random() < 0.5 else np.where(np.arange(n) & 1, a, -a).astype(F32)


def _int16_edge(rng, n):
    vals = np.array([-32768, 32767, 0, -1, 1, -32767], np.int16)
    u = rng.random()
    if u < 0.3:
        return np.full(n, vals[rng.integers(0, 2)], np.int16)
    if u < 0.6:
        return np.where(np.arange(n) & 1, np.int16(32767), np.int16(-32768)).astype(np.int16)
    if u < 0.8:
        return vals[rng.integers(0, len(vals), n)]
    return rng.integers(-32768, 32768, n).astype(np.int16)


def _impulse(rng, n):
    """one sample (sometimes two) on a frame or overlap edge, the rest silence"""
    x = np.zeros(n, F32)
    amps = [1.0, -1.0, BELOW_ONE, 0.5, TINY, -TINY, NORM_MIN, 1e-20, 2.0 ** -15]
    for _ in range(int(rng.integers(1, 3))):
        pos = [EDGES[rng.integers(len(EDGES))] % n, n - 1, 240 * int(rng.integers(0, (n + 239) // 240)) % n][rng.integers(3)]
        x[pos] = amps[rng.integers(len(amps))]
    return x


def _square(rng, n):
    """Nyquist-rate alternation or a full-scale square of a few periods"""
    a = [1.0, BELOW_ONE, 0.5, TINY, 1e-20, 2.0 ** -15][rng.integers(6)]
    half = [1, 1, 1, 2, 8, 16, 120, 240][rng.integers(8)]
    x = np.where((np.arange(n) // half) & 1, -a, a).astype(F32)
    return x if rng.random() < 0.8 else x * F32(-1)


def _dc(rng, n):
    return np.full(n, F32(rng.choice([1.0, -1.0, BELOW_ONE, 0.25, -TINY, 1e-30, 2.0 ** -15])), F32)


def _mixed(rng, n):
    """segments of different kinds: a loud stream range over quiet or subnormal frames"""
    cut = sorted(rng.integers(0, n + 1, 2))
    x = np.zeros(n, F32)
    for (a, b) in ((0, cut[0]), (cut[0], cut[1]), (cut[1], n)):
        if b > a:
            k = KINDS[rng.integers(len(KINDS) - 1)]
            s = k[1](rng, b - a)
            x[a:b] = E.to_float(s)
    return x


KINDS = [("music", _music), ("denormal", _denormal), ("underflow", _underflow), ("signed_zero", _signed_zero), ("unit", _unit),
         ("int16", _int16_edge), ("impulse", _impulse), ("square", _square), ("dc", _dc),
         ("silence", lambda rng, n: np.zeros(n, F32)), ("mixed", _mixed)]
WEIGHTS = np.array([6, 2, 2, 1, 2, 2, 3, 2, 1, 1, 2], float)


def _signal(rng, n):
    name, fn = KINDS[rng.choice(len(KINDS), p=WEIGHTS / WEIGHTS.sum())]
    x = fn(rng, n)
    if x.dtype != np.int16 and name in ("music", "square", "impulse", "dc") and rng.random() < 0.3:
        x = np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    return name, x


def case_set(seed, k, size=10):
    """the k-th set of generator `seed`: `size` cases of one layout (LAYOUTS[k % 10]) and one draw of params"""
    rng = np.random.default_rng([seed, k])
    fam, lay = LAYOUTS[k % len(LAYOUTS)]
    version, (typ, sub) = FAMILIES[fam][0], FAMILIES[fam][1][lay]
    p = _params(rng)
    out = []
    for j in range(size):
        kind, x = _signal(rng, _length(rng))
        out.append(Case("s%d-%d/%d/%s-%s/%s/%d" % (seed, k, j, fam, lay, kind, len(x)), x, fam, lay, version, typ, sub, p))
    return out


# 1-sample streams the GPU test interleaves with a set's cases (one frame each, so a batch's frame count can be made
# anything): silence, full scale, an int16 extreme, a subnormal
FILLS = [np.zeros(1, F32), np.full(1, -1.0, F32), np.full(1, 32767, np.int16), np.full(1, TINY, F32)]


def fillers(seed, k):
    """the 1-sample streams in set k's layout and params"""
    c = case_set(seed, k, 1)[0]
    return [c._replace(name="fill%d-%d/%d/%s-%s" % (seed, k, j, c.family, c.layout), pcm=x) for j, x in enumerate(FILLS)]


def longest(fam):
    """one stream of exactly 65 535 frames for `fam`, at the reference's defaults: a music-like signal with silent, subnormal
    and full-scale stretches"""
    rng = np.random.default_rng([0x10E6, list(FAMILIES).index(fam)])
    x = _music(rng, LONGEST).astype(F32)
    q = LONGEST // 8
    x[q:2 * q] = 0
    x[3 * q:3 * q + 24000] = _denormal(rng, 24000)
    x[5 * q:5 * q + 24000] = _square(rng, 24000)
    version, lays = FAMILIES[fam]
    lay = list(lays)[-1]
    typ, sub = lays[lay]
    return Case("longest/%s-%s" % (fam, lay), x, fam, lay, version, typ, sub, dict(E.DEFAULTS))


def keys(seed, n_sets, with_longest=True, with_fillers=False):
    """the work items of a run: ("long", fam) first (they take longest), then ("set", seed, k) and ("fill", seed, k)"""
    out = [("long", fam) for fam in FAMILIES] if with_longest else []
    return out + [(kind, seed, k) for k in range(n_sets) for kind in (("set", "fill") if with_fillers else ("set",))]


def cases_of(key):
    if key[0] == "long":
        return [longest(key[1])]
    return case_set(key[1], key[2]) if key[0] == "set" else fillers(key[1], key[2])


def run_reference(exe, case, tmp):
    """the reference's bytes and its stderr for one case"""
    src, dst = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.bin")
    E.to_float(case.pcm).astype("<f4").tofile(src)
    p = case.params
    argv = [exe, src, dst, "%x" % case.version, str(case.type), str(case.subtype), float(F32(p["powerBandCutoff"])).hex(),
            str(p["targetBitRate"]), float(F32(p["minimumDynamicRange"])).hex(), float(F32(p["maximumQuantizationError"])).hex()]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s: %s exited %d: %s" % (case.name, os.path.basename(exe), r.returncode, r.stderr[-2000:]))
    with open(dst, "rb") as f:
        return f.read(), r.stderr


def ubsan_kinds(report):
    return sorted({("shift" if "shift" in l else "bounds" if "out of bounds" in l or "index" in l else "float-cast")
                   for l in report.splitlines() if "runtime error" in l})


def restate(case):
    """the restatement's (bytes, (type, sub-type), bandsToKeep, times the Keep +15 rule fired)"""
    if case.family == "94":
        s, win, keep = E.encode(case.pcm, (case.type, case.subtype), **case.params)
        return s, win, keep, 0
    s, typ, keep, fired = R.encode(case.pcm, case.version, case.type, **case.params)
    return s, (typ, 0), keep, fired


Result = collections.namedtuple("Result", "name family layout status kinds ref want win keep fired")


def check(case, with_reference=True):
    """-> Result: status "kept" (the reference's bytes are the contract), "rule" (kept, but the Keep +15 rule fired),
    "dropped" (a bounds or float-cast report) or "unchecked" (no reference); ref = the reference's bytes where kept"""
    want, win, keep, fired = restate(case)
    kinds, ref, status = [], None, "unchecked"
    if with_reference:
        with tempfile.TemporaryDirectory() as tmp:
            _, report = run_reference(SAN, case, tmp)
            kinds = ubsan_kinds(report)
            if any(k != "shift" for k in kinds):
                status = "dropped"
            else:
                ref, _ = run_reference(EXE, case, tmp)
                status = "rule" if fired else "kept"
    return Result(case.name, case.family, case.layout, status, kinds, ref, want, win, keep, fired)


def _check_key(key, with_reference):
    return [check(c, with_reference) for c in cases_of(key)]


def check_all(work, with_reference=True, workers=None):
    """check() every case of the work items, in fresh worker processes (spawned: safe beside an initialised GPU runtime)
    -> {case name: Result}"""
    workers = workers or max(1, min(16, os.cpu_count() or 1))
    out = {}
    ctx = multiprocessing.get_context("spawn")
    with concurrent.futures.ProcessPoolExecutor(workers, mp_context=ctx) as pool:
        for res in pool.map(_check_key, work, [with_reference] * len(work)):
            for r in res:
                out[r.name] = r
    return out


def reference_available():
    return os.path.exists(EXE) and os.path.exists(SAN)


def header_facts(family, stream):
    """what the 16 header bytes show on their own: bandsToKeep (bands past it are 0xFF, kept bands have bit 6 clear) and
    the bits of the winner written in the header of a kept band -> (keep, {field: value})"""
    hdr = stream[2:18]
    keep = next((b for b in range(16) if hdr[b] == 0xFF), 16)
    facts = {}
    if keep > 0:
        facts["type"] = hdr[0] >> 7
    if family == "94":
        if keep > 1:
            facts["sub&2"] = (hdr[1] >> 7) << 1
        if keep > 2:
            facts["sub&1"] = hdr[2] >> 7
    return keep, facts


def tally(results):
    """{(family, layout): {"kept": n, "rule": n, "dropped": n}}"""
    out = {fl: collections.Counter() for fl in LAYOUTS}
    for r in results.values():
        out[r.family, r.layout][r.status] += 1
    return out


def format_tally(t):
    return "\n".join("%-4s %-5s kept %5d  rule %3d  dropped %3d" % (f, l, c["kept"], c["rule"], c["dropped"]) for (f, l), c in t.items())
