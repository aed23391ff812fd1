"""The output-rate converter's restatement and host walk against the compiled libsamplerate (oracle/_ref/dcs_rsout_*, where
`build()` made them), without a GPU, on the seeded cases of tests/rate_out_cases.py: tests/decode_rate_ref.py equals the
binary in samples, count, both clamp counts and the bits of the peak; dcs_resample_out_count and dcs_resample_out_walk equal
the restatement's count and records and the binary's count on every case; at every (table, rate) each length's records are
a prefix of the next longer one's, which is what lets rsOutWalks walk the longest stream of a call alone."""
import collections

import numpy as np
import pytest

import dcsexplorer_amd as D
import decode_rate_ref as Q
import rate_out_cases as C

pytestmark = pytest.mark.skipif(not C.checker_available(), reason=C.MISSING)


@pytest.fixture(scope="module")
def results():
    return C.check_all(C.keys(), with_reference=True, with_restatement=True, with_walks=True)


def all_cases():
    return [c for key in C.keys() for c in C.call_cases(*key)]


def test_the_case_mix(results):
    """conditions on the input and on the reference's output alone; no case is an accident of the seed"""
    dy = C.dyadic_rates()
    print("\ndyadic rates:", dy)
    assert set(dy) | set(C.NEIGHBOURS) | set(C.COMMON) <= set(C.rates("default")) and len(C.rates("default")) >= len(dy) + 10 + 40
    for tab in C.TABLES:
        assert set(dy) | set(C.COMMON) <= set(C.rates(tab)) and len(set(C.rates(tab))) == len(C.rates(tab)) >= len(dy) + 4 + 10
        b = C.buffer_len(tab)
        for rate in C.rates(tab):
            ns = C.lengths(tab, rate)
            assert set(C.NAMED) <= set(ns) and sum(n <= C.MAX_RANDOM_LENGTH and n not in C.NAMED for n in ns) >= 30
            assert (tab == "long") != ({b - 1, b, b + 1, 2 * b + 333} <= set(ns))
        mine = [c for rate in C.rates(tab) for c in C.call_cases(tab, rate)]
        # every kind at every named length, below and above the ring's wrap, and in the host-walked streams
        assert {(c.n, c.kind) for c in mine} >= {(n, k) for n in C.NAMED for k in C.KINDS}
        if tab != "long":
            assert {(c.n, c.kind) for c in mine} >= {(n, k) for n in (b - 1, b, b + 1, 2 * b + 333) for k in C.KINDS}
        routes = collections.Counter(C.host_walked([c.n for c in cases], rate) for rate in C.rates(tab) for _, cases in C.calls(tab, rate))
        assert routes[True] >= 2 and routes[False] >= len(C.rates(tab)), (tab, routes)
    assert C.buffer_len("default") == 30720 and C.buffer_len("long") == 256000
    assert len(C.tables()["big"][0]) == 24578 > C.LDS_MAX_COEFFS >= max(len(C.tables()[t][0]) for t in ("default", "fastest", "long"))
    assert C.clip_condition(results) == []
    # the flush cap binds on the long table from 44.1 kHz up: the walk without it makes more outputs
    c, inc = C.tables()["long"]
    for rate in (44100, 48000, 64000):
        assert Q._walk(4097, len(c), inc, rate, 1 << 30)[0].size > len(results["long/%d/4097/%s" % (rate, dict((x.n, x.kind) for x in C.call_cases("long", rate))[4097])].out)
    # the quiet noise meets the flooring shift: outputs of -1 from values above -1 LSB, and exact ties of the lrint
    lsb = [results[x.name].out for x in all_cases() if x.kind == "lsb"]
    assert sum(int((y == -1).sum()) for y in lsb) > 1000 and sum(int((y == 0).sum()) for y in lsb) > 1000
    print("%d cases in %d calls; per table: %s" % (len(all_cases()), len(C.keys()), dict(collections.Counter(c.table for c in all_cases()))))


def test_restatement_equals_libsamplerate(results):
    bad, rows, thinned = [], collections.Counter(), collections.Counter()
    for c in all_cases():
        r = results[c.name]
        assert (r.want is not None) == C.restated(c)
        if r.want is None:
            thinned[c.table] += 1
            continue
        if np.array_equal(r.want, r.out) and r.want_info == dict(nOut=len(r.out), hi=r.hi, lo=r.lo, peak=r.peak):
            rows[c.table, c.kind] += 1
        else:
            bad.append("%s: %d vs %d samples, clamps %s vs %s, peak %08x vs %08x" % (
                c.name, len(r.want), len(r.out), (r.want_info["hi"], r.want_info["lo"]), (r.hi, r.lo), r.want_info["peak"], r.peak))
    print("\nrestatement == libsamplerate, cases per table and kind (0 set aside; thinned by the cases file's rule: %s):" % dict(thinned))
    for tab in C.TABLES:
        print("%-8s" % tab + "".join(" %s %4d" % (k, rows[tab, k]) for k in C.KINDS))
    assert not bad, "%d cases differ:\n%s" % (len(bad), "\n".join(bad[:20]))
    assert all(sum(rows[t, k] for k in C.KINDS) >= 1000 for t in C.TABLES)
    # nothing the thinning touches is a named edge: every stream of up to 4097 samples was compared
    assert all(results[c.name].want is not None for c in all_cases() if c.n <= 4097)
    # the batched restatement is decode_rate_ref.convert
    for c in all_cases()[5::997]:
        want, info = Q.convert(C.make(c), c.rate, *C.tables()[c.table], Q.AT_UNITY)
        r = results[c.name]
        assert np.array_equal(want, r.out) and info["nClipped"] == r.hi + r.lo and int(info["peak"].view(np.uint32)) == r.peak, c.name


def test_count_walk_and_prefixes_equal_the_restatement(results):
    """every case: the host walk's count is the binary's and the restatement's, its records are the restatement's, and the
    records of each length of a call are a prefix of the next longer one's"""
    n_cases = 0
    for tab, rate in C.keys():
        filt = C.tables()[tab]
        prev = None
        for c in C.call_cases(tab, rate):               # by rising length
            r = results[c.name]
            pos, sfi = D.resample_out_walk(c.n, rate, filt, at_unity=True)
            assert D.resample_out_count(c.n, rate, filt, at_unity=True) == len(pos) == len(r.out) == r.walk[0], c.name
            assert C.walk_digest(pos, sfi) == r.walk, c.name
            if prev is not None:
                assert len(prev[0]) <= len(pos), c.name
                assert np.array_equal(prev[0], pos[:len(prev[0])]) and np.array_equal(prev[1], sfi[:len(prev[1])]), c.name
            prev = (pos, sfi)
            n_cases += 1
    print("\n%d cases: count, walk records and prefixes equal" % n_cases)
    assert n_cases == len(all_cases())
