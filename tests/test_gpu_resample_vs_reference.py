"""dcs_resample_streams and dcs_encode_streams_at on the MI355X against the compiled libsamplerate and the reference encoder
over it (oracle/_ref/dcs_rsref_*, dcs_encrate_ref*, where `build()` made them) on the seeded adversarial cases of
tests/rs_cases.py: the converter's bits on every case of every table -- `big` among them, which is past the LDS variant's
16 384 coefficients and takes rsConvolveKernel<false> -- whatever the batch around a stream; one call of more than 65 535
streams, where every kernel's blockIdx.y loop takes a second pass; long streams at random rates by count and sha256; the
reference encoder's bytes on every case its UBSan build keeps; and the encoder's refusal of a resampled peak above 1
decided by the reference's floats.  Every comparison is equality of bits, bytes, counts or hashes."""
import collections

import numpy as np
import pytest

import dcsexplorer_amd as D
import rs_cases as C
from dcsexplorer_amd.api import ERR_BAD_STREAM

pytestmark = pytest.mark.gpu

SEED = 0x6E52
N_SETS = 45                 # x 15 kinds, 4 fillers each: 9 sets a table, 5 with at_unity and 4 without
N_ENC_SETS = 15             # x 7 kinds: 5 sets a family
N_MANY = 70001
ENC_FMT = {"94": None, "93b": None, "93a": D.FMT_93_T0}


@pytest.fixture(scope="module")
def sets():
    keys = C.keys(SEED, N_SETS, N_ENC_SETS, with_fillers=True, with_long=True, with_many=True, with_peak=True)
    return {key: C.cases_of(key) for key in keys}


@pytest.fixture(scope="module")
def expected(sets):
    return C.check_all(list(sets), with_reference=C.checker_available())


def resample(ctx, cases):
    """one call over cases that share table and flag"""
    c = cases[0]
    got = ctx.resample_streams([x.pcm for x in cases], [x.rate for x in cases], [x.channels for x in cases],
                               filter=C.tables()[c.table], at_unity=c.at_unity)
    assert len(got) == len(cases)
    return got


@pytest.fixture(scope="module")
def resampled(gpu_ctx, sets):
    """every set in one call of its own, in generated order -> {case name: float32 array}"""
    out = {}
    for key, cases in sets.items():
        if key[0] in ("set", "fill"):
            out.update({c.name: y for c, y in zip(cases, resample(gpu_ctx, cases))})
    return out


def _truth(r):
    """the floats a case must give: the reference's, or at the library's own pass-through the downmix"""
    return r.want if r.ref is None else r.ref


def _differs(name, got, r):
    """'' or which of the two the GPU left"""
    ref = "" if r.ref is None or C.same_bits(got, r.ref) else "libsamplerate (%d vs %d samples)" % (len(got), len(r.ref))
    res = "" if C.same_bits(got, r.want) else "the restatement (%d vs %d samples)" % (len(got), len(r.want))
    return "%s differs from %s" % (name, " and ".join(w for w in (ref, res) if w)) if ref or res else ""


def test_gpu_bits_equal_libsamplerate_and_the_restatement(sets, expected, resampled):
    if not C.checker_available():
        pytest.skip(C.MISSING)
    bad, rows = [], []
    for key, cases in sets.items():
        if key[0] != "set":
            continue
        for c in cases:
            d = _differs(c.name, resampled[c.name], expected[c.name])
            if d:
                bad.append(d)
            elif expected[c.name].ref is not None:
                rows.append((c.table, c.kind))
    print("\nGPU == libsamplerate == restatement, cases per table and kind:\n" + C.format_matches(rows))
    assert not bad, "%d GPU streams differ:\n%s" % (len(bad), "\n".join(bad[:20]))
    per_table = collections.Counter(t for t, _ in rows)
    assert all(per_table[t] >= 40 for t in C.TABLES), per_table


def test_gpu_bits_equal_the_restatement(sets, expected, resampled):
    """runs without the checker too: the pass-through cases and the fillers are among these"""
    bad = [c.name for key, cases in sets.items() if key[0] in ("set", "fill") for c in cases
           if not C.same_bits(resampled[c.name], expected[c.name].want)]
    assert not bad, "%d GPU streams differ from the restatement:\n%s" % (len(bad), "\n".join(bad[:20]))


def test_the_big_table_takes_the_global_variant(sets, expected, resampled):
    """three-way equality on a table the LDS variant cannot hold, over every signal kind and rate class"""
    if not C.checker_available():
        pytest.skip(C.MISSING)
    coeffs, inc = C.tables()["big"]
    assert len(coeffs) > 16384 and inc == 512           # kRsLdsMaxCoeffs: a smaller table would go back to LDS
    mine = [c for key, cases in sets.items() if key[0] == "set" for c in cases if c.table == "big"]
    assert {c.kind for c in mine} == set(C.KIND_NAMES) and {c.rate_class for c in mine} == set(C.RATE_CLASSES)
    checked = 0
    for c in mine:
        r = expected[c.name]
        assert not _differs(c.name, resampled[c.name], r)
        checked += r.ref is not None
    assert checked >= 60
    print("\nbig table (%d coefficients): %d cases equal dcs_rsref_big and the restatement" % (len(coeffs), checked))


def _interleave(cases, fills, rng):
    """the cases shuffled, fillers spread between them, and enough more that the call's stream count is a multiple of
    neither 64 nor 256 (the block sizes of the walk and of the stage and convolve kernels)"""
    order = [cases[i] for i in rng.permutation(len(cases))]
    n_fill = len(cases)
    while (len(cases) + n_fill) % 64 == 0 or (len(cases) + n_fill) % 256 == 0:
        n_fill += 1
    out = []
    for i, c in enumerate(order):
        out.append(c)
        out.append(fills[i % len(fills)])
    out += [fills[(i * 3) % len(fills)] for i in range(n_fill - len(cases))]
    assert len(out) % 64 != 0 and len(out) % 256 != 0
    return out


def test_batch_composition(gpu_ctx, sets, expected, resampled):
    """every set shuffled and interleaved with 1- to 3-value streams; two cases of each alone"""
    rng = np.random.default_rng(SEED)
    for key, cases in sets.items():
        if key[0] != "set":
            continue
        mixed = _interleave(cases, sets["fill", key[1], key[2]], rng)
        for c, y in zip(mixed, resample(gpu_ctx, mixed)):
            assert C.same_bits(y, resampled[c.name]) and C.same_bits(y, _truth(expected[c.name])), ("interleaved", c.name)
        for i in rng.choice(len(cases), 2, replace=False):
            assert C.same_bits(resample(gpu_ctx, [cases[i]])[0], resampled[cases[i].name]), ("alone", cases[i].name)


def _many(pool, rng):
    idx = rng.integers(0, len(pool), N_MANY)
    idx[:len(pool)] = np.arange(len(pool))              # every case at least once, and again past stream 65 535
    idx[-len(pool):] = np.arange(len(pool))
    return idx


def test_more_than_65535_streams_in_one_call(gpu_ctx, sets, expected):
    """70 001 streams drawn from 50 short cases: the stage and convolve kernels' blockIdx.y loops take a second pass"""
    pool = sets["many", SEED]
    assert len(pool) == 50 and {c.channels for c in pool} == {1, 2} and len({c.rate for c in pool}) > 10
    idx = _many(pool, np.random.default_rng(SEED + 1))
    assert len(idx) == N_MANY > 65535
    got = resample(gpu_ctx, [pool[i] for i in idx])
    truth = [_truth(expected[c.name]) for c in pool]
    assert all(expected[c.name].ref is not None or c.rate == 31250 for c in pool) or not C.checker_available()
    bad = [(k, pool[i].name) for k, (i, y) in enumerate(zip(idx, got)) if not C.same_bits(y, truth[i])]
    assert not bad, "%d of %d streams differ, first %s" % (len(bad), N_MANY, bad[:5])
    print("\n%d streams in one dcs_resample_streams call: all equal their case's reference bits" % N_MANY)


def test_more_than_65535_streams_through_the_encoder(gpu_ctx, sets, expected):
    pool = sets["many", SEED]
    idx = _many(pool, np.random.default_rng(SEED + 2))
    streams, info = gpu_ctx.encode_streams_at([pool[i].pcm for i in idx], [pool[i].rate for i in idx], 0x9400, None,
                                              channels=[pool[i].channels for i in idx], at_unity=True)
    assert len(streams) == N_MANY
    res = [expected[c.name + "/enc"] for c in pool]
    truth = [r.ref if r.status == "kept" else r.want for r in res]
    bad = [(k, pool[i].name) for k, (i, s) in enumerate(zip(idx, streams)) if s != truth[i] or s != res[i].want]
    assert not bad, "%d of %d streams differ, first %s" % (len(bad), N_MANY, bad[:5])
    if C.checker_available():
        assert sum(r.status == "kept" for r in res) >= 45, collections.Counter(r.status for r in res)
    print("\n%d streams in one dcs_encode_streams_at call: all equal their case's reference bytes" % N_MANY)


def test_long_streams_at_random_rates(gpu_ctx, sets, expected):
    """count and sha256 against the reference, each stream alone and inside a batch of short ones"""
    if not C.checker_available():
        pytest.skip(C.MISSING)
    longs = [cases[0] for key, cases in sets.items() if key[0] == "long"]
    assert len(longs) == len(C.LONG) and any(c.channels == 2 and len(c.pcm) > 2 * 262144 and c.table == "default" for c in longs)
    for c in longs:
        r = expected[c.name]
        alone = resample(gpu_ctx, [c])[0]
        assert (len(alone), C.digest(alone)) == (r.count, r.sha256), ("alone", c.name)
        assert D.resample_count(len(c.pcm), c.rate, c.channels, C.tables()[c.table], at_unity=True) == r.count
        k = next(k for k in range(N_SETS) if C.TABLES[k % len(C.TABLES)] == c.table)       # that table's at_unity set
        around = sets["set", SEED, k]
        batch = around[:7] + [c] + around[7:]
        got = resample(gpu_ctx, batch)
        assert (len(got[7]), C.digest(got[7])) == (r.count, r.sha256), ("in a batch", c.name)
        for b, y in zip(batch, got):
            if b is not c:
                assert C.same_bits(y, _truth(expected[b.name])), ("beside", c.name, b.name)
        print("\n%s: %d samples, sha256 equal alone and in a batch" % (c.name, r.count))


@pytest.fixture(scope="module")
def encoded(gpu_ctx, sets):
    out = {}
    for key, cases in sets.items():
        if key[0] != "enc":
            continue
        c = cases[0]
        streams, info = gpu_ctx.encode_streams_at([x.pcm for x in cases], [x.rate for x in cases], c.version, ENC_FMT[c.family],
                                                  channels=[x.channels for x in cases], at_unity=True)
        out.update({x.name: (s, inf) for x, s, inf in zip(cases, streams, info)})
    return out


def _enc_results(sets, expected):
    return [expected[c.name] for key, cases in sets.items() if key[0] == "enc" for c in cases]


def test_encode_at_equals_the_reference_encoder(sets, expected, encoded):
    if not C.checker_available():
        pytest.skip(C.MISSING)
    res = _enc_results(sets, expected)
    print("\nGPU encoder cases vs dcs_encrate_ref, per family:\n" + C.format_enc_tally(C.enc_tally(res)))
    bad = []
    for r in res:
        got = encoded[r.name][0]
        want = r.ref if r.status == "kept" else r.want         # dropped and rule cases: the library's bytes
        if got != want:
            bad.append("%s (%s): %d vs %d bytes" % (r.name, r.status, len(got), len(want)))
    assert not bad, "%d GPU streams differ:\n%s" % (len(bad), "\n".join(bad[:20]))


def test_encode_at_equals_the_restatements(sets, expected, encoded):
    bad = [r.name for r in _enc_results(sets, expected) if encoded[r.name][0] != r.want]
    assert not bad, bad[:20]
    for name, (s, inf) in encoded.items():
        assert inf["nBytes"] == len(s), name


def test_the_screen_is_not_hollow(sets, expected):
    if not C.checker_available():
        pytest.skip(C.MISSING)
    res = _enc_results(sets, expected)
    t = C.enc_tally(res)
    assert sum(c["kept"] for c in t.values()) >= 0.9 * len(res), C.format_enc_tally(t)
    for fam, c in t.items():
        assert c["kept"] >= 20, (fam, C.format_enc_tally(t))


def test_peak_bookkeeping_follows_the_reference(gpu_ctx, sets, expected):
    """dcs_encode_streams_at refuses exactly the streams whose REFERENCE output leaves [-1, 1] (or is not finite), naming
    the stream, and encodes the rest: subnormal peaks, peaks a few ulps either side of 1, +-inf"""
    if not C.checker_available():
        pytest.skip(C.MISSING)
    cases = sets["peak", SEED]
    ref = {c.name: expected[c.name].ref for c in cases}
    over = {c.name: not bool((np.abs(ref[c.name]) <= 1.0).all()) for c in cases}
    peaks = {c.name: float(np.abs(ref[c.name]).max()) for c in cases}
    inside = [c for c in cases if not over[c.name]]
    outside = [c for c in cases if over[c.name]]
    assert any(np.isinf(peaks[c.name]) for c in outside) and any(1.0 < peaks[c.name] < 1.01 for c in outside)
    assert any(0.99 < peaks[c.name] <= 1.0 for c in inside) and any(0 < peaks[c.name] < C.NORM_MIN for c in inside)
    streams, _ = gpu_ctx.encode_streams_at([c.pcm for c in inside], [c.rate for c in inside])
    assert len(streams) == len(inside) and all(len(s) > 18 for s in streams)
    ok = inside[0]
    for c in outside:
        got = gpu_ctx.resample_streams([c.pcm], [c.rate])[0]
        assert C.same_bits(got, ref[c.name]), c.name
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_streams_at([ok.pcm, ok.pcm, c.pcm, ok.pcm], [ok.rate, ok.rate, c.rate, ok.rate])
        assert e.value.status == ERR_BAD_STREAM and "stream 2" in str(e.value) and "peaks at" in str(e.value), (c.name, str(e.value))
    print("\npeak cases: %d encoded (peaks %s), %d refused (peaks %s)" % (
        len(inside), ", ".join("%.9g" % peaks[c.name] for c in inside), len(outside), ", ".join("%.9g" % peaks[c.name] for c in outside)))
