"""The resampler's host side, without a GPU: the numpy restatement (tests/resample_ref.py) against libsamplerate's own
output run as the reference encoder runs it (tests/golden/resample_golden.*), the encoders' restatements on the resampled
signal against the reference DCSEncoder at other input rates (tests/golden/encode_rate_golden.*), the library's default
filter table (its pinned bits and its stated response), and dcs_resample_count with its argument checks."""
import hashlib
import json
import os

import numpy as np
import pytest

import enc93_ref as E93
import enc_ref as E
import resample_ref as R

import dcsexplorer_amd as D

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = np.load(os.path.join(HERE, "golden", "resample_filters.npz"))
RS = json.load(open(os.path.join(HERE, "golden", "resample_golden.json")))
RS_ARR = np.load(os.path.join(HERE, "golden", "resample_golden.npz"))
ENC = json.load(open(os.path.join(HERE, "golden", "encode_rate_golden.json")))
ENC_ARR = np.load(os.path.join(HERE, "golden", "encode_rate_golden.npz"))
TABLES = ("fastest", "medium", "default", "long")


def table(name):
    return FILTERS[name + "/coeffs"], int(FILTERS[name + "/increment"])


def digest(y):
    return hashlib.sha256(np.asarray(y, "<f4").tobytes()).hexdigest()


def test_golden_covers_the_issue_cases():
    cases = RS["cases"]
    assert {c["table"] for c in cases} == set(TABLES)
    assert {c["rate"] for c in cases} >= {4000, 8000, 11025, 22050, 32000, 44100, 48000, 96000, 384000, 31250}
    assert {c["channels"] for c in cases} == {1, 2}
    assert sum(c["name"] + "/out" in RS_ARR.files for c in cases) >= 100
    assert any(c["count"] == 0 for c in cases)                  # short input at a high rate: no outputs at all
    # the 512-sample cap of the end-of-input flush binds on the long table at 4 kHz
    c, inc = table("long")
    capped = [k for k in cases if k["table"] == "long" and k["rate"] == 4000]
    assert capped
    for k in capped:
        n = len(R.fixture_pcm(RS_ARR, k["signal"]))
        pos, _ = R.walk(n, len(c), inc, 4000)
        assert len(pos) == k["count"] and pos[-1] + R.params(len(c), inc, 4000)[0] >= n
        old, R.FLUSH_CAP = R.FLUSH_CAP, 1 << 30
        try:
            assert R.count(n, 4000, len(c), inc) > k["count"]
        finally:
            R.FLUSH_CAP = old
    # whole seconds at real rates, where the end rule's f64 sum in the converter's own buffer indices drops the last sample
    whole = {(k["table"], k["signal"], k["rate"]): k["count"] for k in cases if k["signal"].startswith("lcg:")}
    assert whole[("default", "lcg:441000:441000:0.5", 44100)] == 312499
    assert whole[("default", "lcg:576000:576000:0.5", 48000)] == 374999
    assert any(k["signal"].startswith("lcg:") for k in ENC["cases"])
    assert {c["version"] for c in ENC["cases"]} == {0x9400, 0x9302, 0x9301}
    assert {c["rate"] for c in ENC["cases"]} >= {4000, 44100, 48000, 384000, 31250}
    assert not ENC["dropped"]


@pytest.mark.parametrize("tab", TABLES)
def test_restatement_reproduces_libsamplerate(tab):
    c, inc = table(tab)
    for k in [k for k in RS["cases"] if k["table"] == tab]:
        y = R.resample(R.fixture_pcm(RS_ARR, k["signal"]), k["rate"], c, inc, k["channels"], R.AT_UNITY)
        assert len(y) == k["count"] and digest(y) == k["sha256"], k["name"]
        if k["name"] + "/out" in RS_ARR.files:
            assert np.array_equal(y.view(np.uint32), RS_ARR[k["name"] + "/out"].view(np.uint32)), k["name"]


@pytest.mark.parametrize("case", ENC["cases"], ids=[c["name"] for c in ENC["cases"]])
def test_encoder_restatements_on_the_restated_resampler(case):
    c, inc = table("default")
    y = R.resample(R.fixture_pcm(ENC_ARR, case["signal"]), case["rate"], c, inc, case["channels"], R.AT_UNITY)
    if case["version"] == 0x9400:
        s = E.encode(y, (case["type"], case["subType"]))[0]
    else:
        s = E93.encode(y, case["version"], case["type"])[0]
    assert len(s) == case["bytes"] and hashlib.sha256(s).hexdigest() == case["sha256"]
    if case["name"] + "/stream" in ENC_ARR.files:
        assert s == ENC_ARR[case["name"] + "/stream"].tobytes()


def test_default_table_keeps_its_bits():
    c, inc = D.resample_filter_default()
    want, want_inc = table("default")
    assert inc == want_inc == 128 and len(c) == 48 * 128 + 2
    assert np.array_equal(c.view(np.uint32), want.view(np.uint32))


def test_default_table_response():
    """the densely sampled prototype (the table mirrored about t = 0, at 128 points per input sample): at least 90 dB down
    from the input's Nyquist frequency on, at most 0.05 dB of ripple up to 0.85 of it, unit gain at DC"""
    c, inc = D.resample_filter_default()
    h = np.concatenate([c[:0:-1], c]).astype(np.float64)
    n = 1 << 19
    mag = np.abs(np.fft.rfft(h, n)) / inc
    f = np.arange(len(mag)) * (2.0 * inc / n)          # in units of the input's Nyquist frequency
    pb, sb = mag[f <= 0.85], mag[f >= 1.0]
    assert 20 * np.log10(pb.max() / pb.min()) <= 0.05
    assert -20 * np.log10(sb.max()) >= 90.0
    assert abs(mag[0] - 1.0) < 1e-4


def test_count_matches_the_restatement():
    for tab in ("fastest", "default", "long"):
        c, inc = table(tab)
        for k in [k for k in RS["cases"] if k["table"] == tab]:
            n = len(R.fixture_pcm(RS_ARR, k["signal"]))
            assert D.resample_count(n, k["rate"], k["channels"], (c, inc), at_unity=True) == k["count"], k["name"]
    c, inc = D.resample_filter_default()
    for n, rate, ch in ((1, 4000, 1), (441000, 44100, 1), (882001, 44100, 2), (7, 384000, 1), (12345, 22050, 2)):
        assert D.resample_count(n, rate, ch) == R.count(n, rate, len(c), inc, ch)
    assert D.resample_count(1000, 31250) == 1000 and D.resample_count(1001, 31250, 2) == 501      # the pass-through
    assert D.resample_count(1000, 31250, at_unity=True) == R.count(1000, 31250, len(c), inc, flags=R.AT_UNITY)


def test_count_argument_errors():
    c, inc = D.resample_filter_default()
    bad = [dict(n_values=100, rate=3999), dict(n_values=100, rate=384001), dict(n_values=0, rate=44100),
           dict(n_values=100, rate=44100, channels=3), dict(n_values=100, rate=44100, channels=0),
           dict(n_values=100, rate=44100, filter=(c[:100], 128)),                 # half length below one increment
           dict(n_values=100, rate=44100, filter=(c, 0)),
           dict(n_values=100, rate=44100, filter=(np.zeros(2, np.float32), 1)),
           dict(n_values=100, rate=44100, filter=(np.where(np.arange(len(c)) == 7, np.inf, c).astype(np.float32), inc)),
           dict(n_values=100, rate=44100, filter=(np.zeros((1 << 19) + 2, np.float32), 128))]
    for kw in bad:
        with pytest.raises(D.DcsError) as e:
            D.resample_count(**kw)
        assert e.value.status == -1, kw
    assert D.resample_count(100, 4000) > 0 and D.resample_count(100, 384000) >= 0
