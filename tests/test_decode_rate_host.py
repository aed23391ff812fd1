"""Decoding at an output rate, the host side, without a GPU: the numpy restatement (tests/decode_rate_ref.py) against
libsamplerate's own output between its own int16 conversions (tests/golden/decode_rate_golden.*, made by
tests/golden/resample/out_rate_driver.c) and, where the reference tree is present, against the freshly built driver on
seeded cases; dcs_resample_out_count and the walk's prefix property (dcs_resample_out_walk) against the restatement; the
argument rules (their messages need a context: tests/test_gpu_decode_rate.py); the FLAC writer's refusals, which this feature leaves as they were."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

import decode_rate_ref as Q

import dcsexplorer_amd as D
from oracle.rsref import big_table

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = np.load(os.path.join(HERE, "golden", "resample_filters.npz"))
GOLD = json.load(open(os.path.join(HERE, "golden", "decode_rate_golden.json")))
GOLD_ARR = np.load(os.path.join(HERE, "golden", "decode_rate_golden.npz"))
TABLES = ("default", "fastest", "medium", "big", "long")
REFERENCE = "/root/reference/libsamplerate/src/src_sinc.c"


def table(name):
    if name == "long":
        return GOLD_ARR["long/coeffs"], int(GOLD_ARR["long/increment"])
    if name == "big":
        return big_table(*table("default"))
    return FILTERS[name + "/coeffs"], int(FILTERS[name + "/increment"])


def digest(y):
    return hashlib.sha256(np.asarray(y, "<i2").tobytes()).hexdigest()


def test_golden_covers_the_issue_cases():
    cases = GOLD["cases"]
    by = {c["name"]: c for c in cases}
    assert {c["table"] for c in cases} == set(TABLES)
    assert {c["rate"] for c in cases} == {4000, 8000, 11025, 22050, 31250, 32000, 44100, 48000, 65535}
    assert {int(c["signal"].split(":")[1]) for c in cases} >= {1, 15, 16, 17, 240, 480, 4080, 4095, 4096, 4097}
    assert {c["signal"].split(":")[0] for c in cases} == {"silence", "dc+", "dc-", "impulse", "square", "noise"}
    assert sum(c["name"] + "/out" in GOLD_ARR.files for c in cases) >= 60
    assert sum(os.path.getsize(os.path.join(HERE, "golden", "decode_rate_golden." + e)) for e in ("json", "npz")) < 200000
    # the clip case clamps in both signs at both of the rates people ask for
    for rate in (44100, 48000):
        c = by["default-%d-square:4080:0" % rate]
        assert c["clippedHigh"] > 0 and c["clippedLow"] > 0
    # 17 frames at 48 kHz: a full FLAC block and a last block of 2 170
    assert by["default-48000-noise:4080:52080"]["count"] == 6266
    # the flush cap binds on the long table: the walk without it goes further
    c, inc = table("long")
    capped = [k for k in cases if k["table"] == "long" and k["rate"] >= 44100 and k["signal"].startswith("noise:4097")]
    assert len(capped) == 3
    for k in capped:
        assert Q.count(4097, k["rate"], len(c), inc) == k["count"]
        old, Q.FLUSH_CAP = Q.FLUSH_CAP, 1 << 30
        try:
            assert Q.count(4097, k["rate"], len(c), inc) > k["count"]
        finally:
            Q.FLUSH_CAP = old


@pytest.mark.parametrize("tab", TABLES)
def test_restatement_reproduces_libsamplerate(tab):
    c, inc = table(tab)
    for k in [k for k in GOLD["cases"] if k["table"] == tab]:
        y, info = Q.convert(Q.case_pcm(k["signal"]), k["rate"], c, inc, Q.AT_UNITY)
        assert len(y) == k["count"] and digest(y) == k["sha256"], k["name"]
        assert info["nClipped"] == k["clippedHigh"] + k["clippedLow"], k["name"]
        assert int(info["peak"].view(np.uint32)) == k["peakBits"], k["name"]
        if k["name"] + "/out" in GOLD_ARR.files:
            assert np.array_equal(y, GOLD_ARR[k["name"] + "/out"]), k["name"]


def test_the_conversions_floor_and_clamp():
    """src_float_to_short_array's rounding, stated on values: the shift floors, and only the two ends are clamped"""
    step = np.float32(1.0 / 32768.0)
    y = np.array([0.0, 0.7 * step, -0.3 * step, step, -step, 32767 * step, 1.0, -1.0, 1.5, -1.5, 32767.99 * step], np.float32)
    out, clipped = Q.float_to_short(y)
    assert out.tolist() == [0, 0, -1, 1, -1, 32767, 32767, -32768, 32767, -32768, 32767]
    assert clipped == 4                                     # 1.0, -1.0, 1.5, -1.5: -1.0 takes the lower branch (v <= -2^31)
    x = np.arange(-32768, 32768).astype(np.int16)
    assert np.array_equal(Q.float_to_short(Q.short_to_float(x))[0], x)
    out, info = Q.convert(x[:500], 31250, *table("default"))
    assert np.array_equal(out, x[:500]) and info["nClipped"] == 0 and info["peak"] == np.float32(1.0)


def test_the_batched_restatement_is_the_restatement():
    """convert_float_many, which tests/rate_out_cases.py runs on a call's streams at once, gives convert_float's bits"""
    for tab, rate in (("default", 48000), ("fastest", 4000), ("long", 62500), ("default", 31250)):
        c, inc = table(tab)
        pcm = [Q.case_pcm(k) for k in ("noise:1:3", "square:240:0", "noise:497:4", "impulse:17:0", "dc-:33:0", "noise:2:5")]
        many = Q.convert_float_many(pcm, rate, c, inc)
        assert len(many) == len(pcm)
        for x, y in zip(pcm, many):
            want = Q.convert_float(x, rate, c, inc)
            assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), want.view(np.uint32)), (tab, rate, len(x))


def seeded_cases(seed=0xD7A1, n_random=12):
    """(table, rate, signal recipe): every rate of the issue's list and seeded other ones, every length, every signal"""
    rng = np.random.default_rng(seed)
    rates = [4000, 8000, 11025, 22050, 31250, 32000, 44100, 48000, 65535] + [int(r) for r in rng.integers(4000, 65536, n_random)]
    lengths = [1, 15, 16, 17, 240, 480, 4080, 4095, 4096, 4097]
    kinds = ["silence", "dc+", "dc-", "impulse", "square", "noise"]
    out = []
    for i, rate in enumerate(rates):
        for j in range(4):
            n = lengths[(3 * i + j * 7 + int(rng.integers(0, 10))) % len(lengths)]
            kind = kinds[(i + j + int(rng.integers(0, 6))) % len(kinds)]
            tab = ("default", "fastest", "medium", "long")[(i + j) % 4]
            out.append((tab, rate, "%s:%d:%d" % (kind, n, 1000 * i + j)))
    # every length and every signal at least once, whatever the draw
    for n in lengths:
        out.append(("default", 48000, "noise:%d:%d" % (n, n)))
    for kind in kinds:
        out.append(("default", 44100, "%s:480:3" % kind))
    return out


@pytest.mark.skipif(not os.path.exists(REFERENCE), reason="the reference tree (libsamplerate's sources) is not on this machine")
def test_restatement_equals_the_freshly_built_driver(tmp_path):
    spec = importlib.util.spec_from_file_location("make_decode_rate_golden", os.path.join(HERE, "golden", "make_decode_rate_golden.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    drv = os.path.join(HERE, "golden", "resample", "out_rate_driver.c")
    exes = {"default": M.build_lsr(str(tmp_path), "default", *table("default"), drv),
            "long": M.build_lsr(str(tmp_path), "long", *table("long"), drv)}
    exes["fastest"] = exes["medium"] = exes["default"]
    cases = seeded_cases()
    assert len(cases) >= 90
    n_clipped = 0
    for tab, rate, key in cases:
        pcm = Q.case_pcm(key)
        want, _ = M.run(exes[tab], pcm, M.CONV[tab], rate, str(tmp_path))
        got, info = Q.convert(pcm, rate, *table(tab), Q.AT_UNITY)
        assert np.array_equal(got, want), (tab, rate, key, len(got), len(want))
        n_clipped += info["nClipped"] > 0
    assert n_clipped >= 3


def test_out_count_equals_the_restatement():
    for tab in TABLES:
        c, inc = table(tab)
        for rate in (4000, 11025, 31250, 44100, 48000, 65535):
            for n in (1, 15, 16, 17, 240, 4080, 4097):
                assert D.resample_out_count(n, rate, (c, inc), at_unity=True) == Q.count(n, rate, len(c), inc, Q.AT_UNITY), (tab, rate, n)
    assert D.resample_out_count(777, 31250) == 777
    assert D.resample_out_count(4080, 48000) == 6266
    for k in GOLD["cases"]:
        n = int(k["signal"].split(":")[1])
        assert D.resample_out_count(n, k["rate"], table(k["table"]), at_unity=True) == k["count"], k["name"]


def test_walk_equals_the_restatement():
    for tab, rate, n in (("default", 48000, 500), ("fastest", 8000, 4097), ("long", 65535, 4097), ("medium", 31250, 17)):
        c, inc = table(tab)
        pos, sfi = D.resample_out_walk(n, rate, (c, inc), at_unity=True)
        want_pos, want_sfi = Q.walk(n, len(c), inc, rate)
        assert np.array_equal(pos, want_pos) and np.array_equal(sfi, want_sfi), (tab, rate, n)


@pytest.mark.parametrize("tab,rate", [("default", 48000), ("default", 44100), ("fastest", 8000), ("fastest", 65535), ("long", 48000),
                                      ("long", 4000), ("default", 31250)])
def test_walk_records_of_a_stream_are_a_prefix_of_a_longer_ones(tab, rate):
    """Output k's record depends on k and the ratio alone; the length decides only the count.  The lengths straddle the
    ring buffer's wrap (its length is buffer_len: the first wrap comes as the loaded samples near it) and, on the long
    table, the flush cap (short streams end before it binds, long ones are cut by it)."""
    c, inc = table(tab)
    b_len = Q.R.buffer_len(len(c), inc)
    lengths = sorted({1, 16, 17, 240, 1000, 4097, b_len - 700, b_len - 1, b_len, b_len + 1, b_len + 5000, 2 * b_len + 333})
    lengths = [n for n in lengths if n >= 1]
    walks = [D.resample_out_walk(n, rate, (c, inc), at_unity=True) for n in lengths]
    for (p1, s1), (p2, s2), n1, n2 in zip(walks, walks[1:], lengths, lengths[1:]):
        assert len(p1) <= len(p2), (n1, n2)
        assert np.array_equal(p1, p2[:len(p1)]) and np.array_equal(s1, s2[:len(s1)]), (n1, n2)
    counts = [len(p) for p, _ in walks]
    assert counts == [D.resample_out_count(n, rate, (c, inc), at_unity=True) for n in lengths]
    if tab == "long" and rate >= 44100:
        # with the cap a long stream falls short of n x ratio by more than the filter's reach would explain without it
        old, Q.FLUSH_CAP = Q.FLUSH_CAP, 1 << 30
        try:
            assert Q.count(4097, rate, len(c), inc) > counts[lengths.index(4097)]
            assert Q.count(16, rate, len(c), inc) == counts[lengths.index(16)]
        finally:
            Q.FLUSH_CAP = old


def test_argument_rules():
    """what is refused, by status.  The messages live in a context's dcs_last_error, and the host-only calls have none:
    tests/test_gpu_decode_rate.py checks the wording where there is a context."""
    for rate in (0, 3999, 65536, 96000):
        with pytest.raises(D.DcsError) as e:
            D.resample_out_count(100, rate)
        assert e.value.status == D.api.ERR_INVALID_ARG
    with pytest.raises(D.DcsError):
        D.resample_out_count(0, 48000)                      # an empty stream
    with pytest.raises(D.DcsError):
        D.resample_out_count(100, 48000, (np.zeros(2, np.float32), 1))         # not a table
    bad = table("default")[0].copy()
    bad[5] = np.nan
    with pytest.raises(D.DcsError):
        D.resample_out_count(100, 48000, (bad, 128))
    L = D.load_library()
    import ctypes
    out = ctypes.c_uint64()
    assert L.dcs_resample_out_count(100, 48000, None, 2, ctypes.byref(out)) != 0        # unknown flag (DCS_OUT_SEQUENCE is the decode calls')
    assert L.dcs_resample_out_count(100, 48000, None, 1, ctypes.byref(out)) == 0
    assert L.dcs_resample_out_count(100, 48000, None, 0, None) != 0
    assert L.dcs_resample_out_count(100, 4000, None, 0, ctypes.byref(out)) == 0 and L.dcs_resample_out_count(100, 65535, None, 0, ctypes.byref(out)) == 0
    assert D.api.OUT_SEQUENCE == 2 and D.RATE_INFO_DTYPE.itemsize == 32


def test_flac_writer_still_refuses_what_it_refused():
    """the writer's argument rules are untouched: whole frames only, no new flag"""
    assert D.flac_write_check([240, 480])[0] == 0
    assert D.flac_write_check([240, 241])[0] != 0
    assert D.flac_write_check([240], flags=4)[0] != 0
