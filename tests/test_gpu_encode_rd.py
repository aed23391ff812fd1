"""The rate-distortion 1994+ encoder on the MI355X (dcs_encode_rd_streams): bytes and every DcsEncodeRdInfo field equal to
the numpy restatement's (tests/enc94rd_ref.py, itself held to the compiled reference decoder and the oracle by
tests/test_encode_rd_host.py), whatever the batch and the groups around a stream; the library's own decoder reads the
streams without an error word; the calling rules are dcs_encode_streams'."""
import ctypes

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc94rd_cases as C
import enc94rd_ref as R
import sweep_ref as S

pytestmark = pytest.mark.gpu


def _fmt(name):
    typ, sub = C.FMTS[name]
    return dict(streamFormatType=typ, streamFormatSubType=sub)


def _check(label, got, inf, infr, want):
    s, ch = want[0], want[1]
    assert C.info_of(infr) == C.info_tuple(ch), label
    assert got == s, label
    assert (inf["formatType"], inf["formatSubType"], inf["nBytes"], inf["bandsToKeep"]) == (ch["type"], ch["sub"], len(s), ch["numBands"]), label
    assert inf["nFrames"] == (s[0] << 8 | s[1])


@pytest.mark.parametrize("name,fmt,rate,mqe", C.GRID, ids=C.IDS)
def test_each_case_alone_equals_the_restatement(gpu_ctx, name, fmt, rate, mqe):
    streams, info, infr = gpu_ctx.encode_rd_streams([C.SIGNALS[name]], None, None, **_fmt(fmt), **C.params(rate, mqe))
    _check(name, streams[0], info[0], infr[0], C.expected(name, fmt, rate, mqe))


FILLS = [np.zeros(1, np.float32), np.full(1, -1.0, np.float32), np.full(1, 32767, np.int16)]


def test_all_cases_in_one_call_shuffled_with_fillers_and_in_small_groups(gpu_ctx, dcs):
    names = list(C.SIGNALS)
    want = {n: C.expected(n, "wild", 96000, C.MQE) for n in names}
    kw = dict(**_fmt("wild"), **C.params(96000, C.MQE))
    streams, info, infr = gpu_ctx.encode_rd_streams([C.SIGNALS[n] for n in names], None, None, **kw)
    for k, n in enumerate(names):
        _check(n, streams[k], info[k], infr[k], want[n])
    # shuffled, a one-frame filler behind each: 32 streams
    rng = np.random.default_rng(0x94D1)
    order = list(rng.permutation(len(names)))
    pcm, where = [], []
    for j, k in enumerate(order):
        where.append(len(pcm))
        pcm += [C.SIGNALS[names[k]], FILLS[j % len(FILLS)]]
    assert len(pcm) == 2 * len(names) == 32
    together, info, infr = gpu_ctx.encode_rd_streams(pcm, None, None, **kw)
    for j, k in enumerate(order):
        _check(names[k], together[where[j]], info[where[j]], infr[where[j]], want[names[k]])
    # groups forced small: 1 job-frame (every job a group of its own), 35 and 70
    try:
        for cap in (1, 35, 70):
            dcs.load_library().dcs_encode_sweep_group_frames(cap)
            again, info2, infr2 = gpu_ctx.encode_rd_streams(pcm, None, None, **kw)
            assert again == together and np.array_equal(info2, info) and np.array_equal(infr2, infr), cap
    finally:
        dcs.load_library().dcs_encode_sweep_group_frames(0)


def test_per_stream_budgets_and_the_rate_form_agree(gpu_ctx):
    names = ["music", "noise_m40", "one_frame", "level_step"]
    budgets = [900, 700, 17, 200]
    kw = dict(**_fmt("T1s3"), **C.params(128000, C.MQE))
    streams, info, infr = gpu_ctx.encode_rd_streams([C.SIGNALS[n] for n in names], None, budgets, **kw)
    for k, n in enumerate(names):
        want = C.expected(n, "T1s3", 128000, C.MQE, budgets[k])
        _check(n, streams[k], info[k], infr[k], want)
        assert len(streams[k]) <= budgets[k] or not infr[k]["fits"]
    assert not infr[2]["fits"] and infr[2]["budgetBits"] == 0
    # a byte budget that names the same bits as a rate: 18 + bits / 8 bytes where the bits are a multiple of 8
    x = C.SIGNALS["noise_m40"]
    bits = 62500 * 17 * 240 // 31250
    assert bits % 8 == 0
    a = gpu_ctx.encode_rd_streams([x], None, None, **_fmt("T0"), **C.params(62500, 0.0))
    b = gpu_ctx.encode_rd_streams([x], None, 18 + bits // 8, **_fmt("T0"), **C.params(1, 0.0))
    assert a[0] == b[0] and np.array_equal(a[2], b[2])


def test_300_frames(gpu_ctx):
    rng = np.random.default_rng(0x300D)
    t = np.arange(240 * 300) / 31250.0
    x = (0.3 * np.sin(2 * np.pi * 440.0 * t) * np.linspace(1, 0.1, len(t)) + rng.normal(0, 0.03, len(t))).clip(-1, 1).astype(np.float32)
    streams, info, infr = gpu_ctx.encode_rd_streams([x, C.SIGNALS["dc"]], D.FMT_94_T1_S3, None, targetBitRate=96000)
    s, ch, _, _ = R.encode(R.analyse(x), (1, 3), None, targetBitRate=96000)
    assert C.info_of(infr[0]) == C.info_tuple(ch) and streams[0] == s and info[0]["nFrames"] == 300


def test_round_trip_through_the_decoder(gpu_ctx, oracle):
    cases = [g for g in C.GRID if g[0] in ("music", "sine_fs", "bands012", "level_step", "one_frame")]
    for name, fmt, rate, mqe in cases:
        s = gpu_ctx.encode_rd_streams([C.SIGNALS[name]], None, None, **_fmt(fmt), **C.params(rate, mqe))[0][0]
        os_ = D.OS95 if (s[3] | s[4]) & 0x80 else D.OS94
        got, err, first = gpu_ctx.decode_streams([(os_, s, 255, 0xFF)], extra_frames=1)
        assert not err.any(), name
        want = oracle.decode(os_, 255, [s], [0xFF], C.FRAMES[name] + 1)
        assert np.array_equal(got, want), name
        assert S.sq_err(S.measure(C.SIGNALS[name], got)) == C.time_error(oracle, os_, C.SIGNALS[name], C.expected(name, fmt, rate, mqe)[0])


def test_calling_rules(gpu_ctx):
    ok = np.zeros(480, np.float32)
    for bad, status in [([np.zeros(0, np.float32)], -1), ([np.zeros(65535 * 240 + 1, np.float32)], -1),
                        ([ok, np.array([0.1, np.nan], np.float32)], -6), ([np.array([np.inf], np.float32)], -6),
                        ([np.array([0.5, 1.0001], np.float32)], -6)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_rd_streams(bad)
        assert e.value.status == status
        with pytest.raises(D.DcsError) as e2:
            gpu_ctx.encode_streams(bad)
        assert e2.value.status == status and str(e2.value) == str(e.value)         # flagged as encode_streams flags them
    for kw in [dict(streamFormatType=2), dict(streamFormatSubType=1), dict(streamFormatSubType=2), dict(formatVersion=0x9301),
               dict(formatVersion=0x9302), dict(targetBitRate=0)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_rd_streams([ok], None, None, **kw)
        assert e.value.status == -1 and "dcs_encode_rd_streams: formatVersion 0x9400" in str(e.value)
    # capacity: too small an output buffer is refused, with the sizes written out
    from dcsexplorer_amd.api import _encode_input, _ptr
    x, offs = _encode_input([ok, C.SIGNALS["noise_m40"]])
    p = D.encode_params(None)
    out_offs = np.zeros(3, np.uint64)
    out = np.zeros(8, np.uint8)
    st = gpu_ctx.L.dcs_encode_rd_streams(gpu_ctx.h, _ptr(x), _ptr(offs), 2, ctypes.byref(p), None, _ptr(out), 8, _ptr(out_offs), None, None)
    assert st == -5
    assert gpu_ctx.L.dcs_encode_rd_streams(gpu_ctx.h, _ptr(x), _ptr(offs), 2, ctypes.byref(p), None, _ptr(out), 8, None, None, None) == -1
    want, _, _ = gpu_ctx.encode_rd_streams([ok, C.SIGNALS["noise_m40"]])
    assert [int(v) for v in out_offs] == [0, len(want[0]), len(want[0]) + len(want[1])] and not out.any()
    # the wildcard never does worse than a layout it contains
    x = C.SIGNALS["music"]
    wild = gpu_ctx.encode_rd_streams([x], None, 600)[2][0]
    for f in (D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3):
        one = gpu_ctx.encode_rd_streams([x], f, 600)[2][0]
        assert wild["sqErr"] <= one["sqErr"] and one["fits"]
    assert gpu_ctx.encode_rd_streams([x], D.FMT_94_T0_S3, 600)[0][0][5:] == gpu_ctx.encode_rd_streams([x], D.FMT_94_T0, 600)[0][0][5:]
    gpu_ctx.encode_rd_streams([np.array([1.0, -1.0] * 300, np.float32)])        # exactly 1.0 and -1.0 are in range
    # the null arguments the entry refuses, and the whole of its parameter message
    one = np.zeros(240, np.float32)
    x, offs = _encode_input([one])
    out_offs = np.zeros(2, np.uint64)
    entry = gpu_ctx.L.dcs_encode_rd_streams
    assert entry(gpu_ctx.h, _ptr(x), None, 1, ctypes.byref(p), None, _ptr(out), 8, _ptr(out_offs), None, None) == -1
    assert entry(gpu_ctx.h, None, _ptr(offs), 1, ctypes.byref(p), None, _ptr(out), 8, _ptr(out_offs), None, None) == -1
    assert entry(None, _ptr(x), _ptr(offs), 1, ctypes.byref(p), None, _ptr(out), 8, _ptr(out_offs), None, None) == -1
    with pytest.raises(D.DcsError) as e:
        gpu_ctx.encode_rd_streams([one], None, None, targetBitRate=0)
    assert str(e.value) == ("libdcs_hip status -1 dcs_encode_rd_streams: formatVersion 0x9400, streamFormatType 0, 1 or -1, "
                            "streamFormatSubType 0, 3 or -1, targetBitRate 1..100 000 000 and finite parameters")
