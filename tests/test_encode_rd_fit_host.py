"""Encoding a set to one byte budget, without a GPU: the library's host allocator (dcs_encode_rd_allot with no context)
against the Python restatement (tests/encrd_fit_ref.py) on seeded curves, the properties DESIGN.md 10.13 states, the fit
calls restated end to end over the two rate-distortion restatements, the quality condition against the per-stream rate
split, and the new record's layout."""
import itertools
import os
import re

import numpy as np
import pytest

import encrd_fit_cases as C
import encrd_fit_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_properties(curves, total, caps, allot, rec, hulls):
    sizes = [int(a) for a in allot]
    assert rec["usedBytes"] == sum(sizes) and rec["leastBytes"] == sum(h[0][0] for h in hulls)
    for j, (a, h) in enumerate(zip(sizes, hulls)):
        assert a in [v[0] for v in h], j                                   # a hull vertex of its job
    if not rec["fits"]:
        assert rec["leastBytes"] > total and sizes == [h[0][0] for h in hulls] and rec["stepsTaken"] == 0
        return
    assert rec["usedBytes"] <= total
    # The remainder only falls.  So a job's next step that fits the remainder now would have fitted at its turn, could not
    # have been the miss that stops its job, and would have been taken: no job's next step fits what is left.
    left = total - rec["usedBytes"]
    for j, (a, h) in enumerate(zip(sizes, hulls)):
        k = [v[0] for v in h].index(a)
        assert k == len(h) - 1 or h[k + 1][0] - a > left, j
    assert rec["sqErr"] == sum(dict(h)[a] for a, h in zip(sizes, hulls))


@pytest.mark.parametrize("name,t,kind", C.GRID, ids=C.IDS)
def test_host_allocator_equals_the_restatement(dcs, name, t, kind):
    curves, total, caps = C.CURVES[name], C.total_of(name, t, kind), C.caps_of(name, kind)
    want, rec, hulls = C.expected(name, t, kind)
    allot, fit = dcs.encode_rd_allot(curves, total, caps)
    assert allot.tolist() == want
    assert FR.record_tuple(fit) == FR.record_tuple(rec)
    assert int(fit["reserved"]) == 0
    _check_properties(curves, total, caps, allot, rec, hulls)


def test_the_cases_reach_what_they_are_for():
    for name, curves in C.CURVES.items():
        hulls = [FR.hull(list(c))[0] for c in curves]
        if name == "non_convex":
            assert any(len(h) < len(c) for h, c in zip(hulls, curves))
        if name == "big_d":
            assert any((h[i][1] - h[i + 1][1]) * (h[i + 1][0] - h[i][0]) > 1 << 64 for h in hulls for i in range(len(h) - 1))
        if name == "many_jobs":
            assert len(curves) == 70000 and {len(c) for c in curves} == {2, 3}
    from fractions import Fraction
    slopes = [Fraction(h[i][1] - h[i + 1][1], h[i + 1][0] - h[i][0]) for c in C.CURVES["slope_ties"]
              for h in [FR.hull(list(c))[0]] for i in range(len(h) - 1)]
    assert len(slopes) - len(set(slopes)) > 10
    # caps that bind, that pin and that lie below 18
    for name in ["mixed", "slope_ties"]:
        caps = C.caps_of(name, "under18")
        pinned = [FR.hull(list(c), cap)[1] for c, cap in zip(C.CURVES[name], caps)]
        assert any(pinned) and not all(pinned) and any(cap < 18 for cap in caps)
        assert any(FR.hull(list(c), cap)[0] != FR.hull(list(c))[0] and not p for c, cap, p in zip(C.CURVES[name], caps, pinned))
    # 64-bit arithmetic would order big_ties differently: the steeper step belongs to the last job
    total = C.total_of("big_ties", 0.37, "none")
    assert C.expected("big_ties", 0.37, "none")[0] == [1 << 31, 1 << 30, (1 << 30) + (1 << 29)] and total < sum([1 << 31, 1 << 30, 1 << 30]) + (1 << 30)


def test_small_sets_against_every_prefix_of_the_slope_order(dcs):
    """Up to 4 jobs of up to 5 points, every total from below the base to the sum of the maxima.  An allocation that uses hull
    vertices only and takes the steps in slope order is a prefix of the ordered step list; the walk takes the longest prefix
    that fits and then goes on, so its error is never above that of any prefix that fits."""
    rng = np.random.default_rng(0xE5A)
    for trial in range(60):
        curves = [[(int(rng.integers(18, 40)), int(rng.integers(0, 50))) for _ in range(int(rng.integers(1, 6)))]
                  for _ in range(int(rng.integers(1, 5)))]
        hulls = [FR.hull(c)[0] for c in curves]
        base, most = sum(h[0][0] for h in hulls), sum(h[-1][0] for h in hulls)
        steps = sorted(((h[i][1] - h[i + 1][1], h[i + 1][0] - h[i][0], j, i) for j, h in enumerate(hulls) for i in range(len(h) - 1)),
                       key=lambda s: (-FR.Fraction(s[0], s[1]), s[2], s[3]))
        for total in range(base - 1, most + 2):
            allot, fit = dcs.encode_rd_allot(curves, total)
            want, rec, _ = FR.allot(curves, total)
            assert allot.tolist() == want and FR.record_tuple(fit) == FR.record_tuple(rec)
            _check_properties(curves, total, None, allot, rec, hulls)
            err, used = sum(h[0][1] for h in hulls), base
            for dd, ds, _, _ in steps:
                if used <= total:
                    assert int(fit["sqErr"]) <= err, (trial, total)
                err -= dd
                used += ds
            if used <= total:
                assert int(fit["sqErr"]) <= err
            # ... and with so few points: never above the best of ALL allocations of hull vertices when the total takes every step
            if total >= most:
                assert int(fit["sqErr"]) == min(sum(d for _, d in pick) for pick in itertools.product(*hulls))


def test_argument_errors(dcs):
    L = dcs.load_library()
    ok = [[(20, 5), (30, 1)]]
    with pytest.raises(dcs.DcsError):
        dcs.encode_rd_allot([[]], 100)                                     # a job without candidates
    with pytest.raises(dcs.DcsError):
        dcs.encode_rd_allot([[(20, 1)] * 169], 100)
    with pytest.raises(dcs.DcsError):
        dcs.encode_rd_allot([[(1 << 32, 1)]], 100)
    with pytest.raises(dcs.DcsError):
        dcs.encode_rd_allot([[(20, 1 << 62)]], 100)
    assert L.dcs_encode_rd_allot(None, None, None, None, 0, 0, None, None, None) != 0
    allot, fit = dcs.encode_rd_allot([], 7)
    assert len(allot) == 0 and FR.record_tuple(fit) == (7, 0, 0, 0, 0, 0, 1)
    allot, fit = dcs.encode_rd_allot(ok, 29)
    assert allot.tolist() == [20] and int(fit["fits"]) == 1


def test_the_record_is_laid_out_as_the_header_says(dcs):
    hdr = open(os.path.join(ROOT, "include", "dcs_hip.h")).read()
    body = re.search(r"typedef struct DcsEncodeRdFitInfo\s*\{(.*?)\}\s*DcsEncodeRdFitInfo;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"\b(u?int(?:32|64)_t)\s+([^;]+);", body):
        for n in names.split(","):
            fields.append((n.strip(), int(re.search(r"\d+", typ).group()) // 8, typ.startswith("u")))
    dt = dcs.ENCODE_RD_FIT_INFO_DTYPE
    assert [f[0] for f in fields] == list(dt.names)
    at = 0
    for name, size, unsigned in fields:
        at = (at + size - 1) // size * size
        assert dt.fields[name][1] == at and dt.fields[name][0].itemsize == size and (dt.fields[name][0].kind == "u") == unsigned, name
        at += size
    assert dt.itemsize == (at + 7) // 8 * 8 == 48
    assert "DCS_ABI_VERSION stays 9" in hdr


# ------------------------------------------------------------------------------------------- the fit calls, restated

FAMILIES = list(C.LAYOUTS94) + C.VERSIONS93
FAMILY_IDS = [f if isinstance(f, str) else "%x" % f for f in FAMILIES]


@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_restated_fit_writes_streams_as_long_as_their_allotments(family):
    for rate in C.RATES:
        total = sum(C.rate_budgets(rate))
        streams, infos, rec, allot = C.expected_fit(family, total)
        assert [len(s) for s in streams] == allot
        assert rec["usedBytes"] == sum(allot) <= total and rec["fits"] == 1
        assert all(i["fits"] and i["budgetBits"] == (a - 18) * 8 for i, a in zip(infos, allot))
    # below the smallest candidates: every stream at its smallest, and still as long as its allotment
    least = C.expected_fit(family, 10 ** 9)[2]["leastBytes"]
    streams, infos, rec, allot = C.expected_fit(family, least - 1)
    assert rec["fits"] == 0 and [len(s) for s in streams] == allot and sum(allot) == least


@pytest.mark.parametrize("rate", C.RATES)
@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_shared_budget_is_never_worse_than_the_rate_split(family, rate):
    """the summed squared error of the shared allocation against that of the per-stream budgets the rate gives, at their sum"""
    total = sum(C.rate_budgets(rate))
    fit, split = C.expected_fit(family, total)[2]["sqErr"], C.expected_split(family, rate)
    print("family %s rate %d: fit %d split %d ratio %.3f" % (family, rate, fit, split, fit / split if split else 1.0))
    assert fit <= split
