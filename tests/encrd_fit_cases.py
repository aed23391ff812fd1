"""Seeded cases of the shared-budget allocator and of the fit calls (test infrastructure): synthetic curves with their totals
and caps, which the host and the GPU tests share, and the ten signals of the fit calls with the restatements' results,
computed once per process."""
import functools

import numpy as np

import enc93rd_ref as R93
import enc94rd_cases as C94
import enc94rd_ref as R94
import encrd_fit_ref as FR

SIGNALS = ["silence", "dc", "sine_fs", "noise_m40", "music", "bands012", "level_step", "one_frame", "band15", "impulse_edge"]
LAYOUTS94 = {"wild": (-1, -1), "T0": (0, 0), "T1s3": (1, 3)}
VERSIONS93 = [0x9301, 0x9302]
RATES = [16000, 32000, 64000, 96000, 128000, 256000]
MQE = C94.MQE


def _curve(rng, n, smax=4000, dmax=1 << 30):
    return [(int(rng.integers(18, smax)), int(rng.integers(0, dmax))) for _ in range(n)]


def _convexish(rng, n):
    """sizes ascending, D descending, neither convex nor strictly either"""
    s = np.cumsum(rng.integers(1, 40, n)) + 18
    d = np.sort(rng.integers(0, 1 << 24, n))[::-1]
    return [(int(a), int(b)) for a, b in zip(s, d)]


def _curves():
    rng = np.random.default_rng(0xF17)
    out = {}
    out["one_job"] = [_curve(rng, 40)]
    out["one_point_jobs"] = [_curve(rng, 1) for _ in range(9)]
    out["mixed"] = [_curve(rng, int(n)) for n in rng.integers(1, 169, 23)]
    out["full_168"] = [_curve(rng, 168, smax=900) for _ in range(5)]
    out["non_convex"] = [_convexish(rng, int(n)) for n in rng.integers(2, 60, 17)]
    c = _curve(rng, 12)
    out["duplicates"] = [c + c[::-1], list(c), [c[3]] * 7, c[:5] + c[:5]]
    # many exact slope ties: sizes and errors small integers, so that steps of different jobs have equal dD / ds
    out["slope_ties"] = [[(18 + int(s), int(d)) for s, d in zip(rng.integers(0, 12, 9), rng.integers(0, 12, 9))] for _ in range(40)]
    out["twin_jobs"] = [[(20, 100), (30, 40), (50, 10)]] * 6
    # products beyond 2^64: D near 2^61, sizes near 2^31
    big = []
    for _ in range(3):                      # (three jobs: the record's sum of errors stays below 2^64)
        n = int(rng.integers(20, 60))
        s = np.sort(rng.integers(18, (1 << 32) - 1, n))
        d = rng.integers(0, (1 << 62) - 1, n)
        big.append([(int(a), int(b)) for a, b in zip(s, d)])
    out["big_d"] = big
    # two steps of equal slope 3 * 2^29 and one steeper by 2^6: the cross products differ by exactly 2^64, so arithmetic cut to
    # 64 bits sees three ties and gives the one step the totals leave room for to another job
    out["big_ties"] = [[(1 << 31, (1 << 61) + 3 * (1 << 59)), ((1 << 31) + (1 << 30), 1 << 61)],
                       [(1 << 30, (1 << 60) + 3 * (1 << 58)), ((1 << 30) + (1 << 29), 1 << 60)],
                       [(1 << 30, (1 << 60) + 3 * (1 << 58) + (1 << 35)), ((1 << 30) + (1 << 29), 1 << 60)]]
    n = 70000
    k = rng.integers(2, 4, n)
    s0, s1, s2 = rng.integers(18, 60, n), rng.integers(1, 50, n), rng.integers(1, 50, n)
    d = rng.integers(0, 1 << 20, (n, 3))
    out["many_jobs"] = [[(int(s0[j]), int(d[j, 0])), (int(s0[j] + s1[j]), int(d[j, 1]))]
                        + ([(int(s0[j] + s1[j] + s2[j]), int(d[j, 2]))] if k[j] == 3 else []) for j in range(n)]
    return out


CURVES = _curves()
# the totals of a case: the base, one below it, the sum of all maxima, and parts of the way between
TOTALS = ["base", "base-1", "max", 0.03, 0.37, 0.81]
LARGE = {"many_jobs"}
# (curves, total, caps): caps None, binding on some jobs, and below 18 on some
GRID = [(name, t, "none") for name in CURVES for t in (TOTALS if name not in LARGE else ["base", 0.37, "max"])]
GRID += [(name, t, caps) for name in ["mixed", "non_convex", "slope_ties", "big_d", "duplicates"] for t in ["max", 0.37, 0.81]
         for caps in ["bind", "under18"]]
IDS = ["%s-%s-%s" % g for g in GRID]


@functools.lru_cache(maxsize=None)
def caps_of(name, kind):
    if kind == "none":
        return None
    rng = np.random.default_rng([0xCA9, len(name)])
    out = []
    for c in CURVES[name]:
        sizes = sorted(p[0] for p in c)
        pick = sizes[int(rng.integers(0, len(sizes)))]
        r = rng.random()
        if kind == "under18" and r < 0.3:
            out.append(int(rng.integers(0, 18)))
        elif r < 0.7:
            out.append(min(pick + int(rng.integers(0, 3)), 0xFFFFFFFF))        # binds unless it picked the largest
        elif r < 0.85:
            out.append(max(sizes[0] - 1, 0))                                    # below every candidate: pinned
        else:
            out.append(0xFFFFFFFF)
    return out


@functools.lru_cache(maxsize=None)
def total_of(name, t, kind):
    hulls = [FR.hull(list(c), None if caps_of(name, kind) is None else caps_of(name, kind)[j])[0] for j, c in enumerate(CURVES[name])]
    base, most = sum(h[0][0] for h in hulls), sum(h[-1][0] for h in hulls)
    if t == "base":
        return base
    if t == "base-1":
        return base - 1
    if t == "max":
        return most
    return base + int((most - base) * t)


@functools.lru_cache(maxsize=None)
def expected(name, t, kind):
    """-> (allotments, record dict, hulls) of the restatement"""
    return FR.allot(CURVES[name], total_of(name, t, kind), caps_of(name, kind))


# ------------------------------------------------------------------------------------------------------- the fit calls

def pcm_list():
    return [C94.SIGNALS[n] for n in SIGNALS]


@functools.lru_cache(maxsize=None)
def analysis93(name, version):
    return R93.analyse(C94.SIGNALS[name], version)


def analyses(family):
    """family: a key of LAYOUTS94, or a version of VERSIONS93"""
    if family in LAYOUTS94:
        return [C94.analysis(n) for n in SIGNALS]
    return [analysis93(n, family) for n in SIGNALS]


def rate_budgets(rate):
    """the per-stream byte budgets a rate gives: 18 header bytes and the whole bytes of floor(rate * frames * 240 / 31250) bits"""
    return [18 + (rate * C94.FRAMES[n] * 240 // 31250) // 8 for n in SIGNALS]


@functools.lru_cache(maxsize=None)
def expected_fit(family, total, caps=None, mqe=MQE):
    """-> (streams, info dicts, record dict, allotments) of the restatement; caps a tuple or None"""
    ans = analyses(family)
    if family in LAYOUTS94:
        return FR.fit94(R94, ans, total, LAYOUTS94[family], caps, maximumQuantizationError=mqe)
    return FR.fit93(R93, ans, total, caps, maximumQuantizationError=mqe)


@functools.lru_cache(maxsize=None)
def expected_split(family, rate, mqe=MQE):
    """the per-stream calls with the rate's budgets -> the summed sqErr"""
    ans = analyses(family)
    if family in LAYOUTS94:
        return sum(R94.encode(an, LAYOUTS94[family], b, maximumQuantizationError=mqe)[1]["sqErr"] for an, b in zip(ans, rate_budgets(rate)))
    return sum(R93.encode(an, b, maximumQuantizationError=mqe)[1]["sqErr"] for an, b in zip(ans, rate_budgets(rate)))


def fit_call(ctx, family, total, pcms=None, cap=None, **params):
    """the library's fit call of a family -> (streams, info, infoRd, record)"""
    import dcsexplorer_amd as D
    pcms = pcm_list() if pcms is None else pcms
    if family in LAYOUTS94:
        fmt = {"wild": None, "T0": D.FMT_94_T0, "T1s3": D.FMT_94_T1_S3}[family]
        return ctx.encode_rd_fit(pcms, total, fmt=fmt, cap=cap, **params)
    return ctx.encode93_rd_fit(pcms, total, os_=D.OS93A if family == 0x9301 else D.OS93B, cap=cap, **params)


def streams_call(ctx, family, budget, pcms=None, **params):
    """the library's per-stream call of a family -> (streams, info, infoRd)"""
    import dcsexplorer_amd as D
    pcms = pcm_list() if pcms is None else pcms
    if family in LAYOUTS94:
        fmt = {"wild": None, "T0": D.FMT_94_T0, "T1s3": D.FMT_94_T1_S3}[family]
        return ctx.encode_rd_streams(pcms, fmt=fmt, budget=budget, **params)
    return ctx.encode93_rd_streams(pcms, os_=D.OS93A if family == 0x9301 else D.OS93B, budget=budget, **params)
