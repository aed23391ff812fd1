"""The rate-distortion OS93 Type-0 encoder on the MI355X (dcs_encode93_rd_streams): bytes and every DcsEncodeRdInfo field
equal to the numpy restatement's (tests/enc93rd_ref.py, itself held to the compiled reference decoder and the oracle by
tests/test_encode93_rd_host.py), whatever the batch and the groups around a stream; the library's own decoder reads the
streams without an error word; the calling rules are dcs_encode93_streams'; the quality condition on the device's bytes."""
import ctypes

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc93rd_cases as C
import enc93rd_ref as R
import sweep_ref as S

pytestmark = pytest.mark.gpu

OS = {C.A: D.OS93A, C.B: D.OS93B}


def _check(label, got, inf, infr, want):
    s, ch = want[0], want[1]
    assert C.info_of(infr) == C.info_tuple(ch), label
    assert got == s, label
    assert (inf["formatType"], inf["formatSubType"], inf["nBytes"], inf["bandsToKeep"]) == (0, 0, len(s), ch["numBands"]), label
    assert inf["nFrames"] == (s[0] << 8 | s[1])


@pytest.mark.parametrize("name,version,rate,mqe", C.GRID, ids=C.IDS)
def test_each_case_alone_equals_the_restatement(gpu_ctx, name, version, rate, mqe):
    streams, info, infr = gpu_ctx.encode93_rd_streams([C.SIGNALS[name]], OS[version], None, **C.params(rate, mqe))
    _check(name, streams[0], info[0], infr[0], C.expected(name, version, rate, mqe))


FILLS = [np.zeros(1, np.float32), np.full(1, -1.0, np.float32), np.full(1, 32767, np.int16)]


@pytest.mark.parametrize("version", [C.A, C.B])
def test_all_cases_in_one_call_shuffled_with_fillers_and_in_small_groups(gpu_ctx, dcs, version):
    names = list(C.SIGNALS)
    want = {n: C.expected(n, version, 96000, C.MQE) for n in names}
    kw = C.params(96000, C.MQE)
    streams, info, infr = gpu_ctx.encode93_rd_streams([C.SIGNALS[n] for n in names], OS[version], None, **kw)
    for k, n in enumerate(names):
        _check(n, streams[k], info[k], infr[k], want[n])
    # shuffled, a one-frame filler behind each
    rng = np.random.default_rng(0x93D1)
    order = list(rng.permutation(len(names)))
    pcm, where = [], []
    for j, k in enumerate(order):
        where.append(len(pcm))
        pcm += [C.SIGNALS[names[k]], FILLS[j % len(FILLS)]]
    together, info, infr = gpu_ctx.encode93_rd_streams(pcm, OS[version], None, **kw)
    for j, k in enumerate(order):
        _check(names[k], together[where[j]], info[where[j]], infr[where[j]], want[names[k]])
    # groups forced small: 1 job-frame (every job a group of its own), 35 and 70
    try:
        for cap in (1, 35, 70):
            dcs.load_library().dcs_encode_sweep_group_frames(cap)
            again, info2, infr2 = gpu_ctx.encode93_rd_streams(pcm, OS[version], None, **kw)
            assert again == together and np.array_equal(info2, info) and np.array_equal(infr2, infr), cap
    finally:
        dcs.load_library().dcs_encode_sweep_group_frames(0)


def test_per_stream_budgets_and_the_rate_form_agree(gpu_ctx):
    names = ["music", "noise_m40", "one_frame", "level_step"]
    budgets = [900, 700, 17, 200]
    kw = C.params(128000, C.MQE)
    streams, info, infr = gpu_ctx.encode93_rd_streams([C.SIGNALS[n] for n in names], D.OS93B, budgets, **kw)
    for k, n in enumerate(names):
        want = C.expected(n, C.B, 128000, C.MQE, budgets[k])
        _check(n, streams[k], info[k], infr[k], want)
        assert len(streams[k]) <= budgets[k] or not infr[k]["fits"]
    assert not infr[2]["fits"] and infr[2]["budgetBits"] == 0
    # a byte budget that names the same bits as a rate: 18 + bits / 8 bytes where the bits are a multiple of 8
    x = C.SIGNALS["noise_m40"]
    bits = 62500 * 17 * 240 // 31250
    assert bits % 8 == 0
    a = gpu_ctx.encode93_rd_streams([x], D.OS93A, None, **C.params(62500, 0.0))
    b = gpu_ctx.encode93_rd_streams([x], D.OS93A, 18 + bits // 8, **C.params(1, 0.0))
    assert a[0] == b[0] and np.array_equal(a[2], b[2])


def test_300_frames(gpu_ctx):
    """more frames than one chunk of the proxy and trellis kernels walks (64), than a block of the offsets scan (256)"""
    rng = np.random.default_rng(0x300D)
    t = np.arange(240 * 300) / 31250.0
    x = (0.3 * np.sin(2 * np.pi * 440.0 * t) * np.linspace(1, 0.1, len(t)) + rng.normal(0, 0.03, len(t))).clip(-1, 1).astype(np.float32)
    streams, info, infr = gpu_ctx.encode93_rd_streams([x, C.SIGNALS["dc"]], D.OS93B, None, targetBitRate=96000)
    s, ch, _, _ = R.encode(R.analyse(x, C.B), None, targetBitRate=96000)
    assert C.info_of(infr[0]) == C.info_tuple(ch) and streams[0] == s and info[0]["nFrames"] == 300
    _check("dc", streams[1], info[1], infr[1], C.expected("dc", C.B, 96000, C.MQE))


def test_round_trip_through_the_decoder(gpu_ctx, oracle):
    cases = [g for g in C.GRID if g[0] in ("music", "sine_fs", "tone700", "level_step", "one_frame", "mid_tone")]
    for name, version, rate, mqe in cases:
        s = gpu_ctx.encode93_rd_streams([C.SIGNALS[name]], OS[version], None, **C.params(rate, mqe))[0][0]
        got, err, first = gpu_ctx.decode_streams([(OS[version], s, 255, 0xFF)], extra_frames=1)
        assert not err.any(), name
        want = oracle.decode(OS[version], 255, [s], [0xFF], C.FRAMES[name] + 1)
        assert np.array_equal(got, want), name


def test_calling_rules(gpu_ctx):
    ok = np.zeros(480, np.float32)
    for bad, status in [([np.zeros(0, np.float32)], -1), ([np.zeros(65535 * 240 + 1, np.float32)], -1),
                        ([ok, np.array([0.1, np.nan], np.float32)], -6), ([np.array([np.inf], np.float32)], -6),
                        ([np.array([0.5, 1.0001], np.float32)], -6)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode93_rd_streams(bad)
        assert e.value.status == status
        with pytest.raises(D.DcsError) as e2:
            gpu_ctx.encode93_streams(bad)
        assert e2.value.status == status and str(e2.value) == str(e.value)         # flagged as encode93_streams flags them
    for kw in [dict(streamFormatType=1), dict(streamFormatType=2), dict(formatVersion=0x9400), dict(targetBitRate=0)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode93_rd_streams([ok], D.OS93B, None, **kw)
        assert e.value.status == -1 and "dcs_encode93_rd_streams: formatVersion 0x9301 or 0x9302" in str(e.value)
    with pytest.raises(D.DcsError) as e:
        gpu_ctx.encode93_rd_streams([ok], D.OS93A, None, streamFormatType=1)
    assert e.value.status == -1 and "dcs_encode93_rd_streams" in str(e.value)
    gpu_ctx.encode93_rd_streams([ok], D.OS93A, None, streamFormatType=-1)
    # capacity: too small an output buffer is refused, with the sizes written out
    from dcsexplorer_amd.api import _encode_input, _ptr
    x, offs = _encode_input([ok, C.SIGNALS["noise_m40"]])
    p = D.encode93_params(D.OS93B, D.FMT_93_T0)
    out_offs = np.zeros(3, np.uint64)
    out = np.zeros(8, np.uint8)
    st = gpu_ctx.L.dcs_encode93_rd_streams(gpu_ctx.h, _ptr(x), _ptr(offs), 2, ctypes.byref(p), None, _ptr(out), 8, _ptr(out_offs), None, None)
    assert st == -5
    assert gpu_ctx.L.dcs_encode93_rd_streams(gpu_ctx.h, _ptr(x), _ptr(offs), 2, ctypes.byref(p), None, _ptr(out), 8, None, None, None) == -1
    want, _, _ = gpu_ctx.encode93_rd_streams([ok, C.SIGNALS["noise_m40"]])
    assert [int(v) for v in out_offs] == [0, len(want[0]), len(want[0]) + len(want[1])] and not out.any()
    gpu_ctx.encode93_rd_streams([np.array([1.0, -1.0] * 300, np.float32)])      # exactly 1.0 and -1.0 are in range
    # the null arguments the entry refuses, and the whole of its parameter message
    one = np.zeros(240, np.float32)
    x, offs = _encode_input([one])
    out_offs = np.zeros(2, np.uint64)
    entry = gpu_ctx.L.dcs_encode93_rd_streams
    assert entry(gpu_ctx.h, _ptr(x), None, 1, ctypes.byref(p), None, _ptr(out), 8, _ptr(out_offs), None, None) == -1
    assert entry(gpu_ctx.h, None, _ptr(offs), 1, ctypes.byref(p), None, _ptr(out), 8, _ptr(out_offs), None, None) == -1
    assert entry(None, _ptr(x), _ptr(offs), 1, ctypes.byref(p), None, _ptr(out), 8, _ptr(out_offs), None, None) == -1
    with pytest.raises(D.DcsError) as e:
        gpu_ctx.encode93_rd_streams([one], D.OS93B, None, targetBitRate=0)
    assert str(e.value) == ("libdcs_hip status -1 dcs_encode93_rd_streams: formatVersion 0x9301 or 0x9302, streamFormatType 0 or -1 "
                            "(OS93 Type 0; Type 1 is not searched), targetBitRate 1..100 000 000 and finite parameters")


def _errors(gpu_ctx, os_, x, streams):
    """per stream (E, E with the decode negated before it is measured)"""
    pcm, err, first = gpu_ctx.decode_streams([(os_, s, 255, 0xFF) for s in streams], extra_frames=1)
    assert not err.any()
    first = list(first) + [pcm.shape[0]]
    d = [np.asarray(pcm[first[k]:first[k + 1]]).astype(np.int64) for k in range(len(streams))]
    return [(S.sq_err(S.measure(x, v)), S.sq_err(S.measure(x, -v))) for v in d]


_QUALITY = {}


def _quality(gpu_ctx, name):
    """rows (version, rate, B, (E, En), bytes, (err, errn), fits) of one signal, computed once: B and E are the length and the
    time-domain error (sweep_ref.measure on the library's own decode) of encode93_streams' Type-0 stream; encode93_rd_streams
    runs with budgetBytes = B.  The device's bytes are the restatement's."""
    if name in _QUALITY:
        return _QUALITY[name]
    x = R.E.to_float(C.quality_signals()[name])
    rows = []
    for version in (C.A, C.B):
        ref = [gpu_ctx.encode93_streams([x], OS[version], D.FMT_93_T0, targetBitRate=rate)[0][0] for rate in S.RATES]
        e_ref = _errors(gpu_ctx, OS[version], x, ref)
        budgets = [len(s) for s in ref]
        got, info, infr = gpu_ctx.encode93_rd_streams([x] * len(S.RATES), OS[version], budgets)
        e_got = _errors(gpu_ctx, OS[version], x, got)
        rows += [(version, rate, budgets[k], e_ref[k], len(got[k]), e_got[k], int(infr[k]["fits"])) for k, rate in enumerate(S.RATES)]
        # (one budget per version, the search being shared by all six)
        want = R.encode(C.quality_analysis(name, version), budgets[2])
        assert got[2] == want[0] and C.info_of(infr[2]) == C.info_tuple(want[1])
    _QUALITY[name] = rows
    return rows


def _show(name, rows, k):
    return ["%-18s %x %6d: B %5d E %13d -> %5d %13d" % (name, v, rate, B, e[k], n, g[k]) for v, rate, B, e, n, g, fits in rows]


@pytest.mark.parametrize("name", C.QUALITY_GPU)
def test_quality_on_the_devices_own_bytes(gpu_ctx, name, capsys):
    """the condition as the issue states it: fits, and the error is never higher than that of encode93_streams' stream, whose
    decode has its polarity turned (tests/test_encode93_rd_vs_reference.py)"""
    rows = _quality(gpu_ctx, name)
    with capsys.disabled():
        print("\n" + "\n".join(_show(name, rows, 0)))
    bad = [r for r in rows if not (r[4] <= r[2] and r[5][0] <= r[3][0] and r[6])]
    assert not bad, _show(name, bad, 0)


@pytest.mark.parametrize("name", C.QUALITY_GPU)
def test_quality_on_the_devices_own_bytes_against_the_reference_with_its_polarity_taken_out(gpu_ctx, name, capsys):
    """encode93_streams' decode negated before it is measured, this encoder's as it comes: the error is never higher, but for
    ec_music0 at 256 and 192 kbit/s, where maximumQuantizationError at its default stops this encoder at 3 676 bytes (the
    host test names the figures)"""
    rows = _quality(gpu_ctx, name)
    with capsys.disabled():
        print("\n" + "\n".join("%-18s %x %6d: B %5d E %13d -> %5d %13d" % (name, v, rate, B, e[1], n, g[0]) for v, rate, B, e, n, g, fits in rows))
    assert all(r[4] <= r[2] and r[6] for r in rows)
    bad = [r for r in rows if r[5][0] > r[3][1] and not (name == "ec_music0" and r[1] in (256000, 192000))]
    assert not bad, _show(name, bad, 0)
