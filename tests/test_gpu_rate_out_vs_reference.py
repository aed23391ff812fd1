"""dcs_resample_out_streams on the MI355X against the compiled libsamplerate (oracle/_ref/dcs_rsout_*, where `build()` made
them) on the seeded cases of tests/rate_out_cases.py, sample for sample, with nOut, nClipped and the bits of the peak: one
call per (table, rate) with every length mixed and shuffled, so that every stream reads a prefix of the record table the
call's longest stream walked; where that table is walked on the host, the rest of the list again as a call a device lane
walks.  The rates are those at which the walk's f64 chain is exact and lands on rounding ties, their neighbours, the common
ones and seeded draws; the lengths lie either side of the converter's ring.  Where the binaries are absent the expected
output is the numpy restatement's (tests/decode_rate_ref.py) on the cases the cases file's thinning rule keeps."""
import collections
import functools

import numpy as np
import pytest

import rate_out_cases as C

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def expected():
    """{case name: Result}, taken once per session in plain CPU child processes and left unchanged"""
    if C.checker_available():
        return C.reference()
    return C.check_all(C.keys(), with_reference=False, with_restatement=True)


def truth(r):
    """(samples, nClipped, peak bits) a case must give, or None where nothing states it"""
    if r.out is not None:
        return r.out, r.hi + r.lo, r.peak
    if r.want is not None:
        return r.want, r.want_info["hi"] + r.want_info["lo"], r.want_info["peak"]
    return None


def routes(table, rate, cases):
    """what a call runs, from the library's own formulas: the convolve kernel by the table's size (kRsLdsMaxCoeffs), the
    walk of the shared record table by rsHostRoute's estimate nIn / step + 4 of the longest stream (kRsHostWalkMin)"""
    return ("LDS convolve" if len(C.tables()[table][0]) <= C.LDS_MAX_COEFFS else "cache convolve",
            "host-walked" if C.host_walked([c.n for c in cases], rate) else "device-walked") + (("at_unity",) if rate == C.IN_RATE else ())


@pytest.mark.parametrize("table", C.TABLES)
def test_every_length_in_one_call(gpu_ctx, table):
    want = expected()
    rng = np.random.default_rng([C.SEED, 9, C.TABLES.index(table)])
    filt = None if table == "default" else C.tables()[table]
    tally, bad, n_checked = collections.Counter(), [], 0
    for rate in C.rates(table):
        for what, cases in C.calls(table, rate):
            cases = [cases[i] for i in rng.permutation(len(cases))]
            out, info = gpu_ctx.resample_out_streams([C.make(c) for c in cases], rate, filt, at_unity=rate == C.IN_RATE)
            assert len(out) == len(cases)
            tally.update(routes(table, rate, cases))
            for c, y, i in zip(cases, out, info):
                t = truth(want[c.name])
                if t is None:
                    continue
                n_checked += 1
                if not (np.array_equal(y, t[0]) and int(i["nIn"]) == c.n and int(i["nOut"]) == len(t[0]) and int(i["nClipped"]) == t[1]
                        and int(i["peak"].view(np.uint32)) == t[2]):
                    bad.append("%s (%s): %d vs %d samples, first difference at %s, clipped %d vs %d, peak %08x vs %08x" % (
                        c.name, what, len(y), len(t[0]), np.flatnonzero(y[:len(t[0])] != t[0][:len(y)])[:1], int(i["nClipped"]), t[1],
                        int(i["peak"].view(np.uint32)), t[2]))
    print("\n%s: %d streams checked against %s; calls by route: %s" % (
        table, n_checked, "the binary" if C.checker_available() else "the restatement", dict(tally)))
    assert not bad, "%d streams differ:\n%s" % (len(bad), "\n".join(bad[:20]))
    assert n_checked >= 1000 and tally["device-walked"] >= len(C.rates(table)) and tally["host-walked"] >= 2 and tally["at_unity"] >= 1


def test_every_route_is_taken():
    tally = collections.Counter(r for t in C.TABLES for rate in C.rates(t) for _, cases in C.calls(t, rate) for r in routes(t, rate, cases))
    print("\ncalls by route:", dict(tally))
    assert all(tally[k] >= 1 for k in ("LDS convolve", "cache convolve", "device-walked", "host-walked", "at_unity")), tally
