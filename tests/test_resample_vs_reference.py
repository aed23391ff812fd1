"""The resampler's restatement and host walk against the compiled libsamplerate (oracle/_ref/dcs_rsref_*, where `build()`
made them), without a GPU, on the seeded adversarial cases of tests/rs_cases.py: tests/resample_ref.py equals the
converter's bits on every short case of every table; dcs_resample_count (the host rsWalk) equals its count on seeded
(length, rate, channels, table) draws up to 2 000 000 values; enc_ref / enc93_ref after resample_ref equal the reference
DCSEncoder over the real converter on every case its UBSan build keeps."""
import collections

import numpy as np
import pytest

import dcsexplorer_amd as D
import rs_cases as C

pytestmark = pytest.mark.skipif(not C.checker_available(), reason=C.MISSING)

SEED = 0x6E52
N_SETS = 45                 # x 15 kinds: 9 sets a table, 5 with at_unity and 4 without (the GPU test's sets)
N_ENC_SETS = 15             # x 7 kinds: 5 sets a family
N_COUNTS = 26               # x 8 draws


@pytest.fixture(scope="module")
def results():
    return C.check_all(C.keys(SEED, N_SETS, N_ENC_SETS, N_COUNTS, with_fillers=True, with_long=True, with_many=True, with_peak=True))


def test_the_case_mix(results):
    """every kind and every rate class on every table, with and without at_unity; no case is an accident of the seed"""
    cases = [c for k in range(N_SETS) for c in C.case_set(SEED, k)]
    for tab in C.TABLES:
        mine = [c for c in cases if c.table == tab]
        assert {c.kind for c in mine} == set(C.KIND_NAMES)
        assert {c.rate_class for c in mine} == set(C.RATE_CLASSES)
        assert {c.at_unity for c in mine} == {True, False}
        assert {c.channels for c in mine} == {1, 2}
        assert any(c.rate == 31250 and c.at_unity for c in mine) and any(c.rate == 31250 and not c.at_unity for c in mine)
    assert len(C.tables()["big"][0]) == 4 * (len(C.tables()["default"][0]) - 2) + 2 > 16384
    # outputs that are subnormal, zero with either sign, and not finite all occur in the reference's floats
    for tab in C.TABLES:
        y = np.concatenate([results[c.name].ref for c in cases if c.table == tab and results[c.name].ref is not None])
        a = np.abs(y)
        assert ((a > 0) & (a < C.NORM_MIN)).sum() > 1000 and np.isinf(y).sum() > 10, tab
        assert (y.view(np.uint32) == 0).any() and ((a > 1e38) & np.isfinite(y)).any(), tab
    # (a sum that starts at +0.0 gives -0.0 only where a negative value underflows in the cast)
    assert any((results[c.name].ref.view(np.uint32) == 0x80000000).any() for c in cases if results[c.name].ref is not None)
    assert any(r.count == 0 for r in results.values() if isinstance(r, C.Result))


def test_restatement_equals_libsamplerate(results):
    bad, rows = [], []
    for r in results.values():
        if not isinstance(r, C.Result) or r.ref is None:
            continue
        if C.same_bits(r.want, r.ref):
            rows.append((r.table, r.kind if r.kind in C.KIND_NAMES else "other"))
        else:
            bad.append("%s: %d vs %d samples" % (r.name, len(r.want), len(r.ref)))
    print("\nrestatement == libsamplerate, cases per table and kind:\n" + C.format_matches(rows))
    assert not bad, "%d cases differ:\n%s" % (len(bad), "\n".join(bad[:20]))
    per_table = collections.Counter(t for t, _ in rows)
    assert all(per_table[t] >= 40 for t in C.TABLES), per_table


def test_host_walk_counts_equal_libsamplerate(results):
    """dcs_resample_count on the count draws, and on every case with reference floats (the long streams among them)"""
    draws = list(results["counts"])
    assert len(draws) >= 200 and max(d[0][0] for d in draws) > 1000000
    assert {d[0][3] for d in draws} == set(C.TABLES) and {d[0][2] for d in draws} == {1, 2}
    for (n, rate, ch, tab), want in draws:
        assert D.resample_count(n, rate, ch, C.tables()[tab], at_unity=True) == want, (n, rate, ch, tab)
    cases = {c.name: c for key in C.keys(SEED, N_SETS, with_fillers=True, with_long=True) for c in C.cases_of(key)}
    n_long = 0
    for name, c in cases.items():
        r = results[name]
        got = D.resample_count(len(c.pcm), c.rate, c.channels, C.tables()[c.table], at_unity=c.at_unity)
        assert got == r.count, name
        n_long += c.kind == "long"
    assert n_long == len(C.LONG)


def test_encoder_restatements_equal_the_reference_encoder(results):
    enc = [r for r in results.values() if isinstance(r, C.EncResult)]
    t = C.enc_tally(enc)
    print("\nencoder cases vs dcs_encrate_ref, per family:\n" + C.format_enc_tally(t))
    bad = [r.name for r in enc if r.status == "kept" and r.want != r.ref]
    assert not bad, bad[:20]
    sets = [r for r in enc if not r.name.endswith("/enc")]
    ts = C.enc_tally(sets)
    assert sum(c["kept"] for c in ts.values()) >= 0.9 * len(sets), C.format_enc_tally(ts)
    assert all(c["kept"] >= 20 for c in ts.values()), C.format_enc_tally(ts)
