"""Seeded adversarial cases for the OS93a Type-1 (pair-table) encoder and its sweep (test infrastructure, no test in it):
layout `93a/T1` beside tests/enc_cases.py's `93a/wild` and `93a/T0`.  Everything is a pure function of (SEED, set index).
A set shares targetBitRate and maximumQuantizationError, so a set is one encoder call; set k takes q = QS[k] and a rate of
enc_cases.RATES, so every q and every rate occurs.  A set holds three signals of enc_cases' kinds (`_signal`, by import) and
its share of the kinds the Type-1 integer rules turn on:

  quiet       noise and tones scaled until the largest |target| is exactly 1, 2, 3, 4, 8 (asserted through
              enc93a_ref.targets): neighbouring scale codes give equal D, candidates tie on sumD, points tie for a pair
  one_band    a tone centred in band b, every b in 0..17 (enc93a_cases' tone_band17 is the recipe); asserted: band b holds
              the most energy
  gaps        loud and all-zero frames interleaved; a stream silent but for one frame; a stream whose every frame reaches
              band 17 (no terminator anywhere at a generous rate)
  ramp        constant frames whose height steps from frame to frame, behind one silent frame: band 0's window start takes,
              for every width, every value a band can have.  (Not every value of 4..0x39-3 is one: reach(w, s) has plateaus
              -- reach(1, s) = 0 0 0 0 1 1 1 1 2 2 3 3 5 5 ... -- so a peak of 1 starts the window of width 1 at 5 and a peak
              of 2 at 9.  Start 4 is the silent band's alone.  ATTAINABLE is the enumeration over every peak 0..32768.)
  low_prv     found by seeded search over the restatement's walks (24 seeded tries: noise a few targets high under one tone
              that a Hann window keeps to its band): a quiet band coded wide and with a low scale code, so that the carried
              prv = s - 2w is below 4, and then a loud band whose window has codes with no delta (delta_value == -1; the
              walk leaves them out).  The three tries with the lowest prv are kept.  Width 9 with scale code 4..7 (prv
              -14..-11) cannot be chosen at all: at codes 4..7 the scale is 1, widths 6..9 then reconstruct the same nine
              points {-1, 0, 1}^2, and the tie goes to fewer bits; and code 4 is in no non-silent band's window (reach(w, 4)
              = 0 < any peak, so hi >= 8).  Width 9 first pays at code 8 (scale 3): prv = -10 is the floor the search can
              approach, and LOW_PRV_MIN records what it reached (-6).
  full_scale  +-1.0 squares and sines at bin centres.  No legal input was found that reaches a target of -32768 or 32767:
              the largest |target| here is the Nyquist square's and DC's 30 959 (FULL_SCALE_PEAK; asserted below 32767), so
              the clamp in `targets` is out of these cases' reach.
  long        256 * 240 and 257 * 240 samples of a quiet tone (enc93aOffsetKernel's carry), once each

Per case two more rates are computed from the restatement: the least rate at which its choice at 10^8 bit/s still fits
(frameBits == budgetBits for streams under 131 frames, where the budget moves a bit at a time), and that rate minus 1.
Q_NEAR_2_64 is one more q, beside the sets': the one whose unbounded error floor comes closest to 2^64 from below.

The restatement's results are computed once per process and cached, as tests/enc93a_cases.py does."""
import collections
import math

import numpy as np

import enc93a_ref as A
import enc_cases as X
from enc93a_cases import fnv1a64  # noqa: F401  (the tests' hash)

F32 = np.float32
SEED = 0x93AF
OS93A = 0
TOP_RATE = 100000000
QS = [float(F32(q)) for q in list(X.MAX_QE) + [k / 32768 for k in range(1, 17)]
      + [1.0, 100.0, 12000.0, 17000.0, 18000.0, 1e6, 1e30, float(np.finfo(F32).max), -2.0]]
N_SETS = len(QS)


def _near_2_64():
    """per band size, the largest binary32 q whose unbounded E_b is still below 2^64; of these the one that comes closest.
    It is the 13-pair band's, 2^36.7 short: an unbounded eb + lambda * bits then wraps for the ladder's entries 61 and 62
    (3 << 30, 2 << 31) from 36 and 27 bits on, while the absent band's 4 bits do not -- a coded band 17 would cost next to
    nothing.  (Wider bands are past 2^64 at this q.)"""
    found = []
    for n in sorted(set(A.INPUTS.tolist())):
        unbounded = lambda q: ((1073741824.0 * float(q)) * float(q)) * float(2 * n)         # noqa: E731
        q = F32(math.sqrt(2.0 ** 64 / (2.0 ** 30 * 2 * n)) * 1.0001)
        while unbounded(q) >= 2.0 ** 64:
            q = np.nextafter(q, F32(0))
        found.append(((1 << 64) - int(unbounded(q)), n, float(q)))
    gap, n, q = min(found)
    assert n == 13 and gap < A.LADDER[62] * 27 and gap > A.LADDER[62] * 4
    return q


Q_NEAR_2_64 = _near_2_64()
RANDOM_PER_SET = 3
MAX_FRAMES = 1500
INFO_KEYS = ("selector", "ladderIndex", "numBands", "frameBits", "budgetBits", "sqErr")

Case = collections.namedtuple("Case", "name kind pcm set rate q")


def rate_of(k):
    return X.RATES[(5 * k + 3) % len(X.RATES)]


def spectrum(pcm):
    """the targets [F, 254] of a signal"""
    return A.targets(A.E.analyse(A.E.frames_of(A.E.to_float(pcm))))


def _tone_at(word, amp, n):
    """a tone at the centre of frame-buffer word `word` (word i holds f[i - 1], 256 bins over 0..15 625 Hz)"""
    return (amp * np.sin(2 * np.pi * ((word - 0.5) / 256 * 15625) * np.arange(n) / 31250)).astype(F32)


def _scaled_to_peak(x0, peak, words=254):
    """x0 * a with the largest |target| of the first `words` words exactly `peak` (bisection on a; the peak grows with a)"""
    lo, hi = 0.0, 64.0
    for _ in range(60):
        a = (lo + hi) / 2
        p = int(np.abs(spectrum((x0 * a).astype(F32))[:, :words]).max())
        if p == peak:
            return (x0 * a).astype(F32)
        lo, hi = (a, hi) if p < peak else (lo, a)
    raise AssertionError("no scale gives a peak of %d" % peak)


def _quiet():
    rng = np.random.default_rng([SEED, 0x71])
    out = []
    for peak in (1, 2, 3, 4, 8):
        noise = rng.standard_normal(480) * 1e-3
        tone = np.sin(2 * np.pi * rng.uniform(300, 9000) * np.arange(480) / 31250) * 1e-3 + rng.standard_normal(480) * 1e-4
        for tag, x0 in (("noise", noise), ("tone", tone)):
            x = _scaled_to_peak(x0, peak)
            assert int(np.abs(spectrum(x)).max()) == peak
            out.append(("quiet/%s_peak%d" % (tag, peak), x))
    return out


def _one_band():
    out = []
    for b in range(18):
        x = _tone_at(2 * int(A.FIRST[b]) + int(A.INPUTS[b]), 0.5, 240 - 3 * b)
        t = spectrum(x)
        e = [int((t[:, 2 * A.FIRST[k]:2 * (A.FIRST[k] + A.INPUTS[k])] ** 2).sum()) for k in range(18)]
        assert int(np.argmax(e)) == b, (b, e)
        out.append(("one_band/%02d" % b, x))
    return out


def _gaps():
    rng = np.random.default_rng([SEED, 0x6A])
    loud = (rng.standard_normal(240 * 6) * 0.2).clip(-1, 1).astype(F32)
    inter = loud.copy()
    for f in (1, 3, 4):                                     # frame k is x[240k - 16 .. 240k + 240): silent with its overlap
        inter[240 * f - 16:240 * (f + 1)] = 0
    t = spectrum(inter)
    silent = [f for f in range(6) if not t[f].any()]
    assert silent == [1, 3, 4], silent
    lonely = np.zeros(240 * 8, F32)
    n = np.arange(200)
    lonely[240 * 3 + 10:240 * 3 + 210] = (0.4 * np.hanning(200) * np.sin(2 * np.pi * 60 * n / 31250 + 1.0)).astype(F32)
    t = spectrum(lonely)
    assert [f for f in range(8) if t[f].any()] == [3]
    n = np.arange(240 * 4)
    every17 = (_tone_at(241, 0.4, len(n)) + rng.standard_normal(len(n)) * 0.01).astype(F32)
    return [("gaps/interleaved", inter), ("gaps/lonely", lonely), ("gaps/every17", every17)]


# per width: {window start: the smallest peak that gives it}, over every peak there is
def _attainable(w):
    starts, first = np.unique(A.window_start(np.arange(32769), w), return_index=True)
    return dict(zip(starts.tolist(), first.tolist()))


ATTAINABLE = [{}] + [_attainable(w) for w in range(1, 10)]


def _ramp():
    """one frame per smallest peak of every attainable window start, rising; frame 0 silent.  The last 16 samples of every
    frame are zero, so no frame overlaps the next and each is scaled to its peak on its own.  The frames are constant:
    nothing else within +-1.0 takes band 0 as high (see full_scale)"""
    frame = np.ones(240)
    frame[224:] = 0
    top = int(np.abs(spectrum(frame.astype(F32))[:, :4]).max())
    peaks = sorted({p for w in range(1, 10) for p in ATTAINABLE[w].values() if 0 < p <= top})
    assert peaks[-1] == max(max(ATTAINABLE[w].values()) for w in range(1, 10))     # every start there is, of every width
    x = np.concatenate([np.zeros(240, F32)] + [_scaled_to_peak(frame * (p / top), p, 4) for p in peaks])
    assert np.abs(x).max() <= 1
    return x


def _ramp_case():
    x = _ramp()
    peak = np.abs(spectrum(x)[:, :4]).max(axis=1)
    for w in range(1, 10):
        assert set(A.window_start(peak, w).tolist()) == set(ATTAINABLE[w]), w
    assert {4, A.S_MAX - 3} <= set(A.window_start(peak, 1).tolist())
    return [("ramp/steps", x)]


def _full_scale():
    n = np.arange(480)
    out = [("full_scale/square_half%d" % h, np.where((n // h) & 1, -1.0, 1.0).astype(F32)) for h in (1, 2, 8, 120)]
    out += [("full_scale/sine_word%d" % w, _tone_at(w, 1.0, 480)) for w in (3, 100, 250)]
    out.append(("full_scale/dc", np.ones(480, F32)))
    return out


def _long():
    rng = np.random.default_rng([SEED, 0x10])
    out = []
    for nf in (256, 257):
        n = np.arange(240 * nf)
        out.append(("long/%d" % nf, (0.01 * np.sin(2 * np.pi * 440 * n / 31250) + rng.standard_normal(len(n)) * 1e-4).astype(F32)))
    return out


def walk_int(D0, S0, D, pp, lam, Eb):
    """one frame, one candidate, in Python integers and stated as a minimum, not as a loop that replaces: among the absent
    band and every reachable (w <= Wmax(pp), s in S), the least (cost, bits, w, s).  D0 [18], S0 [18][10], D [18][10][NS]
    -> dict(w, s, L, through, sumD, prv: the lowest carried, unreachable: window codes with no delta, bit_ties: bands whose
    winner shares its cost with an option of other bits, full_ties: ... with an option of the same bits)"""
    prv, bits = A.PRV0, 0
    o = dict(w=[], s=[], L=-1, through=0, sumD=0, prv=A.PRV0, unreachable=0, bit_ties=0, full_ties=0)
    for b in range(18):
        n, eb = int(A.INPUTS[b]), int(Eb[b])
        opts = [(max(int(D0[b]), eb) + lam * int(A.PFX_LEN[pp][0]), int(A.PFX_LEN[pp][0]), 0, 0, int(D0[b]))]
        for w in range(1, A.WMAX[pp] + 1):
            for k in range(A.NS):
                s = int(S0[b][w]) + k
                v = s - (prv + 2 * w - 1)
                v = v + 54 if v < 0 else v
                if v < 0 or v > 53:
                    o["unreachable"] += 1
                    continue
                nb = int(A.PFX_LEN[pp][w]) + int(A.DL_LEN[v]) + n * w
                opts.append((max(int(D[b][w][k]), eb) + lam * nb, nb, w, s, int(D[b][w][k])))
        cost, nb, w, s, d = min(opts)
        o["bit_ties"] += any(x[0] == cost and x[1] != nb for x in opts)
        o["full_ties"] += sum(x[0] == cost and x[1] == nb for x in opts) > 1
        bits += nb
        o["sumD"] += d
        if w:
            prv = s - 2 * w
            o["prv"] = min(o["prv"], prv)
            o["L"], o["through"] = b, bits
        o["w"].append(w)
        o["s"].append(s)
    return o


def walks_of(an, q, c):
    """walk_int of candidate c on every frame of an analysis"""
    D0, S0, D = (v.tolist() for v in an["search"])
    Eb = [int(e) for e in A.band_floor(q)]
    return [walk_int(D0[f], S0[f], D[f], c // A.KL, A.LADDER[c % A.KL], Eb) for f in range(len(D0))]


LOW_PRV_TRIES = 24
LOW_PRV_KEEP = 3


def _low_prv():
    """a tone under a Hann window over the 256 samples of frame 1 (a stationary tone's skirt would raise the bands around it
    step by step, and prv with them), over noise a few targets high: quiet bands coded at low scale codes, then one loud band"""
    rng = np.random.default_rng([SEED, 0x109])
    found = []
    for j in range(LOW_PRV_TRIES):
        b = int(rng.integers(6, 18))
        pair = int(A.FIRST[b] + rng.integers(3, A.INPUTS[b]))
        x = rng.standard_normal(480) * rng.uniform(5e-5, 4e-4)
        x[224:480] += rng.uniform(0.3, 1.0) * np.hanning(256) * np.sin(2 * np.pi * pair * np.arange(256) / 256 + rng.uniform(0, 6))
        x = x.astype(F32)
        an = A.analyse(x)
        _, ch, _ = A.encode_type1(an, targetBitRate=TOP_RATE, maximumQuantizationError=0.0)
        ws = walks_of(an, 0.0, ch["selector"] * A.KL + ch["ladderIndex"])
        found.append((min(w["prv"] for w in ws), -sum(w["unreachable"] for w in ws), j, x))
    found.sort(key=lambda r: r[:3])
    kept = found[:LOW_PRV_KEEP]
    assert any(r[1] < 0 for r in kept), "no kept case has a window code without a delta"
    return [("low_prv/try%02d" % j, x) for _, _, j, x in kept], kept[0][0]


# Where the special kinds go, by the q of the set (QS[k]) and its rate: the quiet noises under the least q (0, 2^-149, 1e-40,
# 1/32768, 3/32768), the quiet tones under q = 1/32768 .. 5/32768, where E_b = k^2 * 2 * inputs is of their D's size; the loud ones half under the large q (q = 1.0 puts E_b at 2^30 * 2 * inputs,
# beside a full-scale band's D); gaps, ramp and low_prv under the least q, so that their bands are coded
HOMES = dict(quiet=[0, 11, 1, 12, 2, 13, 3, 14, 4, 15], one_band=list(range(27, 36)) + [3, 4, 5, 6, 7, 8, 9, 10, 21],
             gaps=[1, 0, 2], ramp=[2], low_prv=[0, 5, 12], full_scale=[27, 8, 28, 29, 30, 31, 32, 33], long=[14, 21])


def _build():
    low, low_min = _low_prv()
    special = _quiet() + _one_band() + _gaps() + _ramp_case() + low + _full_scale() + _long()
    peak = max(int(np.abs(spectrum(x)).max()) for name, x in special if name.startswith("full_scale/"))
    assert peak < 32767
    cases, sets, home, nth = {}, [], {}, collections.Counter()
    for name, _ in special:
        kind = name.split("/")[0]
        home[name] = HOMES[kind][nth[kind]]
        nth[kind] += 1
    for k in range(N_SETS):
        rng = np.random.default_rng([SEED, k])
        names = []
        for j in range(RANDOM_PER_SET):
            kind, x = X._signal(rng, int(X.LENGTHS[rng.integers(len(X.LENGTHS))]))
            names.append(("s%d/%d/%s/%d" % (k, j, kind, len(x)), kind, x))
        names += [(name, name.split("/")[0], x) for name, x in special if home[name] == k]
        for name, kind, x in names:
            assert x.dtype == np.int16 or (np.isfinite(x).all() and np.abs(x).max() <= 1), name          # legal input only
            cases[name] = Case(name, kind, x, k, rate_of(k), QS[k])
        sets.append([n[0] for n in names])
    return cases, sets, low_min, peak


CASES, SETS, LOW_PRV_MIN, FULL_SCALE_PEAK = _build()
NAMES = list(CASES)
FRAMES = {n: (len(c.pcm) + 239) // 240 for n, c in CASES.items()}
assert sum(FRAMES.values()) <= MAX_FRAMES, sum(FRAMES.values())
assert sorted(FRAMES[n] for n in NAMES if n.startswith("long/")) == [256, 257]
assert {rate_of(k) for k in range(N_SETS)} == set(X.RATES)
_AN, _RES = {}, {}


def params(rate, q):
    return dict(targetBitRate=int(rate), maximumQuantizationError=float(F32(q)))


def analysis(name):
    if name not in _AN:
        _AN[name] = A.analyse(CASES[name].pcm)
    return _AN[name]


def walk(name, q):
    an = analysis(name)
    key = float(F32(q))
    if key not in an["walks"]:
        an["walks"][key] = A.walk(*an["search"], key)
    return an["walks"][key]


def type1(name, rate=None, q=None):
    """the restated Type-1 stream of a case, at its set's rate and q unless given -> (bytes, info93a dict, reconstruction)"""
    c = CASES[name]
    rate, q = c.rate if rate is None else rate, c.q if q is None else q
    key = (name, int(rate), float(F32(q)))
    if key not in _RES:
        _RES[key] = A.encode_type1(analysis(name), **params(rate, q))
    return _RES[key]


def type0(name, rate=None, q=None):
    """the restated Type-0 side (tests/enc93_ref.py) -> (bytes, type, bandsToKeep, ...)"""
    c = CASES[name]
    rate, q = c.rate if rate is None else rate, c.q if q is None else q
    key = (name, int(rate), float(F32(q)), "t0")
    if key not in _RES:
        _RES[key] = A.E93.encode(analysis(name)["x"], 0x9301, 0, **dict(A.DEFAULTS, **params(rate, q)))
    return _RES[key]


def expected(name, typ, rate=None, q=None):
    """what encode93a_streams must return -> (bytes, type written, bandsToKeep, info93a dict); typ 1 or -1: the wildcard
    takes the first strictly smallest, Type 0 first"""
    s, ch, _ = type1(name, rate, q)
    if typ == 1:
        return s, 1, ch["numBands"], ch
    t0 = type0(name, rate, q)
    return (s, 1, ch["numBands"], ch) if len(s) < len(t0[0]) else (t0[0], 0, t0[2], ch)


def candidates(wk):
    """[(sumD, frameBits, candidate, numBands)] of a stream's 256 candidates"""
    out = []
    for c in range(4 * A.KL):
        L = wk["L"][:, c]
        nb = max(1, 1 + int(L.max()))
        out.append((int(wk["sumD"][:, c].sum()), int(wk["through"][:, c].sum()) + 4 * int((L + 1 < nb).sum()), c, nb))
    return out


def edge_rates(name):
    """(the least rate at which the case's choice at TOP_RATE still fits, that rate - 1)"""
    fb = type1(name, TOP_RATE)[1]["frameBits"]
    per = FRAMES[name] * 240
    r = -((-fb * 31250) // per)
    assert A.budget_bits(r, FRAMES[name]) >= fb > A.budget_bits(r - 1, FRAMES[name]) and 2 <= r <= TOP_RATE
    return r, r - 1


def point_ties(name, rate=None, q=None):
    """pairs of the emitted stream whose nearest point is not alone at its distance"""
    s, ch, _ = type1(name, rate, q)
    c = CASES[name]
    wk = walk(name, c.q if q is None else q)
    cand = ch["selector"] * A.KL + ch["ladderIndex"]
    t, n_ties = analysis(name)["t"], 0
    for f in range(t.shape[0]):
        for b in range(int(wk["L"][f, cand]) + 1):
            w, sc = int(wk["w"][f, cand, b]), int(wk["s"][f, cand, b])
            if w == 0:
                continue
            lo, n = 2 * A.FIRST[b], A.INPUTS[b]
            tb = t[f, lo:lo + 2 * n].reshape(n, 2)
            d = ((tb[:, None, :] - A.recon(A.pairs_of(w) * A.SFS[sc])[None, :, :]) ** 2).sum(axis=2)
            n_ties += int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    return n_ties


def facts(name, rate=None, q=None):
    """what a case's restated encode went through: the chosen candidate walked again by walk_int (which must agree with the
    numpy walk), and the ties the choice and the emit met"""
    c = CASES[name]
    rate, q = c.rate if rate is None else rate, c.q if q is None else q
    s, ch, _ = type1(name, rate, q)
    wk = walk(name, q)
    cand = ch["selector"] * A.KL + ch["ladderIndex"]
    ws = walks_of(analysis(name), q, cand)
    for f, o in enumerate(ws):
        assert o["w"] == wk["w"][f, cand].tolist() and o["s"] == wk["s"][f, cand].tolist(), (name, f)
        assert (o["L"], o["through"], o["sumD"]) == (int(wk["L"][f, cand]), int(wk["through"][f, cand]), int(wk["sumD"][f, cand])), (name, f)
    cands = candidates(wk)
    pool = [x for x in cands if x[1] <= ch["budgetBits"]] if ch["fits"] else cands
    last = [o["L"] for o in ws]
    return dict(bit_ties=sum(o["bit_ties"] for o in ws), full_ties=sum(o["full_ties"] for o in ws),
                unreachable=sum(o["unreachable"] for o in ws), prv=min(o["prv"] for o in ws),
                sumd_ties=sum(x[0] == ch["sqErr"] for x in pool) - 1 if ch["fits"] else 0,
                point_ties=point_ties(name, rate, q), no_terminator=all(L + 1 == ch["numBands"] for L in last),
                one_band_coded=ch["numBands"] == 1 and max(last) == 0, selector=ch["selector"], fits=ch["fits"])


def enc_case(name, rate=None, q=None):
    """the case as enc_cases.check takes it: layout 93a/T0, the wildcard's other side"""
    c = CASES[name]
    p = dict(A.DEFAULTS, **params(c.rate if rate is None else rate, c.q if q is None else q))
    p = {k: int(v) if k == "targetBitRate" else float(F32(v)) for k, v in p.items()}
    return X.Case(name, c.pcm, "93a", "T0", 0x9301, 0, -1, p)


def dec_case(name, stream, extra=1):
    """an encoder-made stream as dec_cases.run_reference takes it"""
    import dec_cases                                        # (it loads the package: only where a decoder case is made)
    return dec_cases.Case(name, OS93A, 255, [(0xFF, stream)], extra, "enc93a", ())
