"""Encoding a set to one byte budget on the MI355X (dcs_encode_rd_fit, dcs_encode93_rd_fit, dcs_encode_rd_allot with a
context): the device allocator equal to the host one on every synthetic case; the fit calls' bytes, records and allotments
equal to the restatement's (tests/encrd_fit_ref.py over enc94rd_ref / enc93rd_ref) and to the per-stream calls given the
allotments, whatever the order and the groups; the edges; the library's decoder on what was written; the calling rules."""
import ctypes

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc93rd_ref as R93
import enc94rd_cases as C94
import enc94rd_ref as R94
import encrd_fit_cases as C
import encrd_fit_ref as FR

pytestmark = pytest.mark.gpu

FAMILIES = list(C.LAYOUTS94) + C.VERSIONS93
FAMILY_IDS = [f if isinstance(f, str) else "%x" % f for f in FAMILIES]
FIT_RATES = [16000, 64000, 256000]
FILLS = [np.zeros(1, np.float32), np.full(1, -1.0, np.float32), np.full(1, 32767, np.int16)]


def _info_of(rec):
    return C94.info_of(rec)


def _check_fit(label, got, want, caps=None):
    streams, info, infr, fit = got
    w_streams, w_infos, w_rec, w_allot = want
    assert [len(s) for s in streams] == w_allot, label
    assert FR.record_tuple(fit) == FR.record_tuple(w_rec), label
    for j, (s, ch) in enumerate(zip(w_streams, w_infos)):
        assert _info_of(infr[j]) == C94.info_tuple(ch), (label, j)
        assert streams[j] == s, (label, j)
        assert (info[j]["formatType"], info[j]["formatSubType"], info[j]["nBytes"], info[j]["bandsToKeep"]) \
            == (ch["type"], ch["sub"], len(s), ch["numBands"]), (label, j)


@pytest.mark.parametrize("name,t,kind", C.GRID, ids=C.IDS)
def test_device_allocator_equals_the_host_one(gpu_ctx, name, t, kind):
    curves, total, caps = C.CURVES[name], C.total_of(name, t, kind), C.caps_of(name, kind)
    want, wfit = D.encode_rd_allot(curves, total, caps)
    got, fit = D.encode_rd_allot(curves, total, caps, ctx=gpu_ctx)
    assert np.array_equal(got, want)
    assert fit.tobytes() == wfit.tobytes()
    assert got.tolist() == C.expected(name, t, kind)[0]


@pytest.mark.parametrize("family", FAMILIES, ids=FAMILY_IDS)
def test_fit_equals_the_restatement_and_the_per_stream_call(gpu_ctx, family):
    for rate in FIT_RATES:
        total = sum(C.rate_budgets(rate))
        got = C.fit_call(gpu_ctx, family, total)
        want = C.expected_fit(family, total)
        _check_fit((family, rate), got, want)
        again = C.streams_call(gpu_ctx, family, want[3])
        assert again[0] == got[0] and np.array_equal(again[1], got[1]) and np.array_equal(again[2], got[2]), (family, rate)


@pytest.mark.parametrize("family", ["wild", 0x9302], ids=["wild", "9302"])
def test_shuffled_with_fillers_and_in_forced_groups(gpu_ctx, dcs, family):
    rng = np.random.default_rng(0xF172)
    order = list(rng.permutation(len(C.SIGNALS)))
    pcm = []
    for j, k in enumerate(order):
        pcm += [C94.SIGNALS[C.SIGNALS[k]], FILLS[j % len(FILLS)]]
    total = sum(C.rate_budgets(64000)) + 40 * len(order)
    together = C.fit_call(gpu_ctx, family, total, pcms=pcm)
    assert [len(s) for s in together[0]] == [int(v) for v in together[1]["nBytes"]]
    assert int(together[3]["usedBytes"]) == sum(len(s) for s in together[0]) <= total and int(together[3]["fits"]) == 1
    per = C.streams_call(gpu_ctx, family, [len(s) for s in together[0]], pcms=pcm)
    assert per[0] == together[0] and np.array_equal(per[2], together[2])
    try:
        for cap in (1, 35, 70):
            dcs.load_library().dcs_encode_sweep_group_frames(cap)
            again = C.fit_call(gpu_ctx, family, total, pcms=pcm)
            assert again[0] == together[0] and np.array_equal(again[1], together[1]) and np.array_equal(again[2], together[2]), cap
            assert again[3].tobytes() == together[3].tobytes(), cap
    finally:
        dcs.load_library().dcs_encode_sweep_group_frames(0)


def test_of_a_twin_pair_the_lower_index_takes_the_step(gpu_ctx):
    x = C94.SIGNALS["music"]
    h = FR.hull(FR.curve94(R94, C94.analysis("music"), (0, 0), C.MQE))[0]
    assert len(h) >= 3
    total = 2 * h[0][0] + (h[1][0] - h[0][0])
    streams, info, infr, fit = gpu_ctx.encode_rd_fit([x, x], total, fmt=D.FMT_94_T0)
    assert [len(s) for s in streams] == [h[1][0], h[0][0]]
    assert int(fit["stepsTaken"]) == 1 and int(fit["usedBytes"]) == total and int(fit["nSteps"]) == 2 * (len(h) - 1)
    assert [int(v) for v in infr["sqErr"]] == [h[1][1], h[0][1]]
    # one byte short of the second twin's step changes nothing; with that byte both twins stand on the second vertex
    ds = h[1][0] - h[0][0]
    assert [len(s) for s in gpu_ctx.encode_rd_fit([x, x], total + ds - 1, fmt=D.FMT_94_T0)[0]] == [h[1][0], h[0][0]]
    assert [len(s) for s in gpu_ctx.encode_rd_fit([x, x], 2 * h[1][0], fmt=D.FMT_94_T0)[0]] == [h[1][0], h[1][0]]


@pytest.mark.parametrize("family", ["T1s3", 0x9301], ids=["T1s3", "9301"])
def test_edges(gpu_ctx, family):
    huge = C.expected_fit(family, 10 ** 9)
    least = huge[2]["leastBytes"]
    # a total under the smallest candidates: every stream at its smallest, DCS_OK, fits = 0
    got = C.fit_call(gpu_ctx, family, least - 1)
    _check_fit("under", got, C.expected_fit(family, least - 1))
    assert int(got[3]["fits"]) == 0 and int(got[3]["usedBytes"]) == least and all(int(f) == 1 for f in got[2]["fits"])
    # a huge total: what the per-stream call writes with huge budgets
    got = C.fit_call(gpu_ctx, family, 10 ** 9)
    _check_fit("huge", got, huge)
    per = C.streams_call(gpu_ctx, family, 0xFFFFFFFF)
    assert per[0] == got[0] and [int(v) for v in per[2]["sqErr"]] == [int(v) for v in got[2]["sqErr"]]
    # a cap that binds one stream, and a cap of 17 on another: pinned, its own fits 0
    total = sum(C.rate_budgets(64000))
    free = C.expected_fit(family, total)[3]
    k = C.SIGNALS.index("music")
    caps = [0xFFFFFFFF] * len(C.SIGNALS)
    caps[k] = free[k] - 1
    caps[C.SIGNALS.index("noise_m40")] = 17
    got = C.fit_call(gpu_ctx, family, total, cap=caps)
    want = C.expected_fit(family, total, tuple(caps))
    _check_fit("caps", got, want, caps)
    assert len(got[0][k]) < free[k] and int(got[2][k]["fits"]) == 1
    pinned = got[2][C.SIGNALS.index("noise_m40")]
    assert int(pinned["fits"]) == 0 and int(pinned["budgetBits"]) == 0 and int(got[3]["fits"]) == 1


def test_round_trip_through_the_decoder(gpu_ctx, oracle):
    total = sum(C.rate_budgets(64000))
    for family, os_of in [("wild", lambda s: D.OS95 if (s[3] | s[4]) & 0x80 else D.OS94), (0x9302, lambda s: D.OS93B)]:
        streams = C.fit_call(gpu_ctx, family, total)[0]
        batch = [(os_of(s), s, 255, 0xFF) for s in streams]
        got, err, first = gpu_ctx.decode_streams(batch, extra_frames=1)
        assert not err.any(), family
        for name in ["music", "sine_fs", "level_step"]:
            j = C.SIGNALS.index(name)
            n = C94.FRAMES[name] + 1
            want = oracle.decode(batch[j][0], 255, [streams[j]], [0xFF], n)
            assert np.array_equal(got[first[j]:first[j] + n], want), (family, name)


def test_calling_rules(gpu_ctx):
    ok = np.zeros(480, np.float32)
    for bad, status in [([np.zeros(0, np.float32)], -1), ([np.zeros(65535 * 240 + 1, np.float32)], -1),
                        ([ok, np.array([0.1, np.nan], np.float32)], -6), ([np.array([0.5, 1.0001], np.float32)], -6)]:
        for fit, per in [(gpu_ctx.encode_rd_fit, gpu_ctx.encode_rd_streams), (gpu_ctx.encode93_rd_fit, gpu_ctx.encode93_rd_streams)]:
            with pytest.raises(D.DcsError) as e:
                fit(bad, 1000)
            with pytest.raises(D.DcsError) as e2:
                per(bad)
            assert e.value.status == status == e2.value.status and str(e.value) == str(e2.value)
    for kw in [dict(streamFormatType=2), dict(streamFormatSubType=1), dict(formatVersion=0x9301), dict(targetBitRate=0)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_rd_fit([ok], 1000, **kw)
        assert e.value.status == -1 and "dcs_encode_rd_fit: formatVersion 0x9400" in str(e.value)
    for kw in [dict(streamFormatType=1), dict(formatVersion=0x9400), dict(targetBitRate=0)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode93_rd_fit([ok], 1000, **kw)
        assert e.value.status == -1 and "dcs_encode93_rd_fit: formatVersion 0x9301 or 0x9302" in str(e.value)
    # no streams: zeros, and a record that fits
    streams, info, infr, fit = gpu_ctx.encode_rd_fit([], 5)
    assert streams == [] and FR.record_tuple(fit) == (5, 0, 0, 0, 0, 0, 1)
    # capacity: too small an output buffer is refused, with the offsets (and the record) written and nothing else
    from dcsexplorer_amd.api import _encode_input, _ptr
    pcms = [ok, C94.SIGNALS["noise_m40"]]
    x, offs = _encode_input(pcms)
    for entry, call, p in [(gpu_ctx.L.dcs_encode_rd_fit, gpu_ctx.encode_rd_fit, D.encode_params(None)),
                           (gpu_ctx.L.dcs_encode93_rd_fit, gpu_ctx.encode93_rd_fit,
                            D.encode_params(None, formatVersion=0x9302, streamFormatType=0, streamFormatSubType=0))]:
        out_offs = np.zeros(3, np.uint64)
        out = np.zeros(8, np.uint8)
        info, infr = np.zeros(2, D.ENCODE_INFO_DTYPE), np.zeros(2, D.ENCODE_RD_INFO_DTYPE)
        fit = np.zeros(1, D.ENCODE_RD_FIT_INFO_DTYPE)
        st = entry(gpu_ctx.h, _ptr(x), _ptr(offs), 2, ctypes.byref(p), 700, None, _ptr(out), 8, _ptr(out_offs), _ptr(info), _ptr(infr), _ptr(fit))
        assert st == -5
        assert entry(gpu_ctx.h, _ptr(x), _ptr(offs), 2, ctypes.byref(p), 700, None, _ptr(out), 8, None, None, None, None) == -1
        want = call(pcms, 700)
        assert [int(v) for v in out_offs] == [0, len(want[0][0]), len(want[0][0]) + len(want[0][1])]
        assert not out.any() and not info.tobytes().strip(b"\0") and not infr.tobytes().strip(b"\0")
        assert int(fit[0]["usedBytes"]) == int(out_offs[2]) == int(want[3]["usedBytes"])
    # the null arguments the entries refuse, and the whole of their parameter messages
    one = np.zeros(240, np.float32)
    x, offs = _encode_input([one])
    out_offs = np.zeros(2, np.uint64)
    for entry, p in [(gpu_ctx.L.dcs_encode_rd_fit, D.encode_params(None)),
                     (gpu_ctx.L.dcs_encode93_rd_fit, D.encode_params(None, formatVersion=0x9302, streamFormatType=0, streamFormatSubType=0))]:
        assert entry(gpu_ctx.h, _ptr(x), None, 1, ctypes.byref(p), 700, None, _ptr(out), 8, _ptr(out_offs), None, None, None) == -1
        assert entry(gpu_ctx.h, None, _ptr(offs), 1, ctypes.byref(p), 700, None, _ptr(out), 8, _ptr(out_offs), None, None, None) == -1
        assert entry(None, _ptr(x), _ptr(offs), 1, ctypes.byref(p), 700, None, _ptr(out), 8, _ptr(out_offs), None, None, None) == -1
    with pytest.raises(D.DcsError) as e:
        gpu_ctx.encode_rd_fit([one], 1000, targetBitRate=0)
    assert str(e.value) == ("libdcs_hip status -1 dcs_encode_rd_fit: formatVersion 0x9400, streamFormatType 0, 1 or -1, "
                            "streamFormatSubType 0, 3 or -1, targetBitRate 1..100 000 000 and finite parameters")
    with pytest.raises(D.DcsError) as e:
        gpu_ctx.encode93_rd_fit([one], 1000, targetBitRate=0)
    assert str(e.value) == ("libdcs_hip status -1 dcs_encode93_rd_fit: formatVersion 0x9301 or 0x9302, streamFormatType 0 or -1 "
                            "(OS93 Type 0; Type 1 is not searched), targetBitRate 1..100 000 000 and finite parameters")
