"""Budgets from any source on the MI355X (dcs_encode_streams_at_budget, dcs_transcode_streams_budget,
dcs_encode_files_budget).  The expected bytes come from the restatement (tests/budget_chain_ref.py, pinned in
tests/golden/budget_chain_golden.json) and from the composition of the calls that existed before: resample_streams,
wav_decode, flac_decode and decode_streams, then encode_rd_streams / encode93_rd_streams or their _fit calls.  Never from
the call under test."""
import ctypes
import json
import os

import numpy as np
import pytest

import budget_chain_ref as B
import dcsexplorer_amd as D
import dcsexplorer_amd.api as A
import encrd_fit_ref as FR
import transcode_ref as T
from test_gpu_transcode import _bad_source, _sources

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "budget_chain_golden.json")))
VERSIONS = B.VERSIONS
IDS = ["%x" % v for v in VERSIONS]
RATE = 32000                    # the rate whose per-file budgets the shared totals add up


def _fmt(version):
    return D.FMT_94_T0 if version == 0x9400 else None


def _searched(ctx, version, pcms, budget=None, total=None, cap=None, **params):
    """the calls that existed, on floats at 31 250 Hz -> (streams, info, infoRd[, fit])"""
    if version == 0x9400:
        if total is None:
            return ctx.encode_rd_streams(pcms, fmt=_fmt(version), budget=budget, **params)
        return ctx.encode_rd_fit(pcms, total, fmt=_fmt(version), cap=cap, **params)
    if total is None:
        return ctx.encode93_rd_streams(pcms, os_=B.OS_OF[version], budget=budget, **params)
    return ctx.encode93_rd_fit(pcms, total, os_=B.OS_OF[version], cap=cap, **params)


def _same(got, want, label):
    assert got[0] == want[0], label
    assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes(), label
    if len(want) > 3:
        assert got[-1].tobytes() == want[-1].tobytes(), label


def _decoded(ctx, s, os_):
    pcm, err, _ = ctx.decode_streams([(os_, s, 0x67, 0xFF)], extra_frames=1)
    assert not err.any()
    return pcm.ravel().astype(np.float32) / np.float32(32768)


def _composed(ctx, version, units, budget=None, total=None, cap=None, **params):
    """units as budget_chain_ref.run takes them, through the calls that existed: the copies first, the searched jobs with
    their share -> (streams, infoRd tuples, record tuple or None)"""
    n = len(units)
    searched = [j for j in range(n) if units[j][0] == "pcm"]
    streams, infos = [bytes(u[1]) if u[0] == "copy" else None for u in units], [B.COPY_INFO] * n
    rec = None
    if total is None:
        if searched:
            r = _searched(ctx, version, [units[j][1] for j in searched], None if budget is None else [budget[j] for j in searched], **params)
    else:
        copies = sum(len(units[j][1]) for j in range(n) if units[j][0] == "copy")
        least = used = sq = steps = taken = 0
        if searched:
            r = _searched(ctx, version, [units[j][1] for j in searched], total=max(total - copies, 0),
                          cap=None if cap is None else [cap[j] for j in searched], **params)
            least, used, sq, steps, taken = (int(r[3][k]) for k in ("leastBytes", "usedBytes", "sqErr", "nSteps", "stepsTaken"))
        rec = (total, least + copies, used + copies, sq, steps, taken, int(least + copies <= total))
    for k, j in enumerate(searched):
        streams[j], infos[j] = r[0][k], B.info_of(r[2][k])
    return streams, infos, rec


def _check_units(got, want, label):
    streams, infos, rec = want[:3]
    assert got[0] == streams, label
    assert [B.info_of(r) for r in got[2]] == [tuple(int(v) for v in i) for i in infos], label
    if rec is not None:
        assert FR.record_tuple(got[-1]) == (FR.record_tuple(rec) if isinstance(rec, dict) else rec), label


# ------------------------------------------------------------------------------------------------------- any-rate PCM

def _pcm_list():
    rng = np.random.default_rng(0xB0D6)
    def sig(n, amp=0.5):
        return (amp * (0.7 * np.sin(np.arange(n) * 0.05) + 0.3 * (rng.random(n) * 2 - 1))).astype(np.float32)
    # (values, rate, channels): 3 frames passed through; under 240 samples from 44.1 kHz stereo; one frame from 8 kHz; 3 frames
    # from 44.1 kHz mono and from 8 kHz stereo; under 240 samples passed through in stereo
    return [(sig(720), 31250, 1), (sig(2 * 330), 44100, 2), (sig(60), 8000, 1), (sig(1000), 44100, 1), (sig(2 * 150), 8000, 2),
            (sig(2 * 200), 31250, 2)]


@pytest.mark.parametrize("shared", [False, True], ids=["per-job", "shared"])
@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_any_rate_pcm_equals_resample_then_search(gpu_ctx, version, shared):
    src = _pcm_list()
    pcm, rates, ch = [s[0] for s in src], [s[1] for s in src], [s[2] for s in src]
    floats = gpu_ctx.resample_streams(pcm, rates, ch)
    assert [(len(x) + 239) // 240 for x in floats] == [3, 1, 1, 3, 3, 1] and len(floats[1]) < 240 and len(floats[5]) < 240
    budgets = [18 + 40 * ((len(x) + 239) // 240) for x in floats]
    kw = dict(total=sum(budgets), cap=[10 ** 6, 10 ** 6, 17, 10 ** 6, 10 ** 6, 10 ** 6]) if shared else dict(budget=budgets)
    got = gpu_ctx.encode_streams_at_budget(pcm, rates, version, _fmt(version), channels=ch, **kw)
    _same(got, _searched(gpu_ctx, version, floats, **kw), (version, shared))
    if shared:
        # the cap of 17 pins its job, and reports fits = 0 for it alone
        assert [int(f) for f in got[2]["fits"]] == [1, 1, 0, 1, 1, 1] and int(got[3]["fits"]) == 1
        assert sum(len(s) for s in got[0]) == int(got[3]["usedBytes"]) <= sum(budgets)
    else:
        rate = gpu_ctx.encode_streams_at_budget(pcm, rates, version, _fmt(version), channels=ch, targetBitRate=48000)
        _same(rate, _searched(gpu_ctx, version, floats, targetBitRate=48000), (version, "rate"))
    # the restatement on the same floats
    want = B.run(version, [("pcm", x) for x in floats], **kw)
    _check_units(got, want, (version, shared, "restated"))


@pytest.mark.parametrize("version", [0x9400, 0x9302], ids=["9400", "9302"])
def test_level_fit_encodes_what_level_off_refuses(gpu_ctx, version):
    # a full-scale square wave at 44.1 kHz: the converter's ringing takes its peak past 1
    x = np.where((np.arange(1200) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)
    lvl = D.Level(D.LEVEL_FIT, ceiling=1.0)
    floats, linfo = gpu_ctx.resample_streams([x], 44100, level=lvl)
    assert float(linfo[0]["peakIn"]) > 1.0 >= float(linfo[0]["peakOut"])
    for kw in (dict(budget=[200]), dict(total=230)):
        got = gpu_ctx.encode_streams_at_budget([x], 44100, version, _fmt(version), level=lvl, **kw)
        want = _searched(gpu_ctx, version, floats, **kw)
        assert got[0] == want[0] and got[2].tobytes() == want[2].tobytes() and got[3].tobytes() == linfo.tobytes()
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_streams_at_budget([x], 44100, version, _fmt(version), **kw)
        assert e.value.status == A.ERR_BAD_STREAM and "stream 0: the resampled signal peaks at |x| = " in str(e.value)


# ---------------------------------------------------------------------------------------------------- existing streams

def _stream_call(ctx, srcs, version, **kw):
    return ctx.transcode_streams_budget([s for s, _ in srcs], [o for _, o in srcs], version, _fmt(version), **kw)


def _stream_call_fmt(ctx, srcs, version, fmt, **kw):
    return ctx.transcode_streams_budget([s for s, _ in srcs], [o for _, o in srcs], version, fmt, **kw)


def _stream_units(ctx, srcs, version, budget=None, total=None, cap=None, reencode_all=False):
    units = []
    for j, (s, os_) in enumerate(srcs):
        if B.copied(T.action(s, os_, version) == T.COPIED, len(s), j, budget, total, cap, reencode_all):
            units.append(("copy", s))
        else:
            units.append(("pcm", _decoded(ctx, s, os_)))
    return units


@pytest.mark.parametrize("reencode_all", [False, True], ids=["copy", "all"])
@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_every_layout_into_every_target(gpu_ctx, version, reencode_all):
    srcs = _sources(0x7B0 + VERSIONS.index(version))
    assert [T.frames(s) for s, _ in srcs] == [17 + 6 * k for k in range(6)]
    lens = [len(s) for s, _ in srcs]
    copyable = [T.action(s, o, version) == T.COPIED for s, o in srcs]
    assert any(copyable) and not all(copyable)
    # budgets at every source's own length (what can be copied is), and one byte below it (nothing is)
    for delta in (0, -1):
        budget = [n + delta for n in lens]
        got = _stream_call(gpu_ctx, srcs, version, budget=budget, reencode_all=reencode_all)
        units = _stream_units(gpu_ctx, srcs, version, budget=budget, reencode_all=reencode_all)
        assert [u[0] == "copy" for u in units] == [c and delta == 0 and not reencode_all for c in copyable]
        plan, bound = D.transcode_plan_budget([s for s, _ in srcs], [o for _, o in srcs], version, _fmt(version), reencode_all, budget=budget)
        assert [int(a) for a in plan] == [int(a) for a in got[1]["action"]] == [T.COPIED if u[0] == "copy" else T.REENCODED for u in units]
        _check_units(got, _composed(gpu_ctx, version, units, budget=budget), (version, reencode_all, delta))
        for k, ((s, _), out, inf) in enumerate(zip(srcs, got[0], got[1])):
            assert len(out) <= int(bound[k]) and int(inf["enc"]["nBytes"]) == len(out) and int(inf["srcFrames"]) == T.frames(s)
            if units[k][0] == "copy":
                assert out == s and int(inf["enc"]["bandsToKeep"]) == -1 and B.info_of(got[2][k]) == B.COPY_INFO      # verbatim
            else:
                assert T.frames(out) == T.frames(s) + 1 and int(inf["enc"]["nFrames"]) == T.frames(s) + 1
                assert len(out) <= budget[k] or not int(got[2][k]["fits"])
    # no budgets given: what can be copied is, the others at the rate's bits
    got = _stream_call(gpu_ctx, srcs, version, reencode_all=reencode_all)
    units = _stream_units(gpu_ctx, srcs, version, reencode_all=reencode_all)
    _check_units(got, _composed(gpu_ctx, version, units), (version, reencode_all, "rate"))


@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_shared_total_that_the_copies_nearly_exhaust_and_exceed(gpu_ctx, version):
    srcs = _sources(0x7C0 + VERSIONS.index(version))
    units = _stream_units(gpu_ctx, srcs, version, total=1)
    copies = sum(len(u[1]) for u in units if u[0] == "copy")
    n_s = sum(u[0] == "pcm" for u in units)
    assert copies and n_s
    huge = _stream_call(gpu_ctx, srcs, version, total=10 ** 9)
    least = int(huge[3]["leastBytes"])
    for total in (least + 7, least, least - 1, copies + 1, copies - 1):
        got = _stream_call(gpu_ctx, srcs, version, total=total)
        _check_units(got, _composed(gpu_ctx, version, units, total=total), (version, total))
        assert int(got[3]["totalBytes"]) == total and int(got[3]["fits"]) == int(total >= least)
        assert int(got[3]["usedBytes"]) == sum(len(s) for s in got[0])
        assert [s for s, u in zip(got[0], units) if u[0] == "copy"] == [u[1] for u in units if u[0] == "copy"]
        if total < least:
            # every searched job at its first vertex
            assert int(got[3]["usedBytes"]) == least
    # a cap below a copyable source's length has it searched
    k = [u[0] for u in units].index("copy")
    cap = [10 ** 6] * len(srcs)
    cap[k] = len(srcs[k][0]) - 1
    got = _stream_call(gpu_ctx, srcs, version, total=10 ** 9, cap=cap)
    assert int(got[1][k]["action"]) == T.REENCODED and len(got[0][k]) < len(srcs[k][0])
    _check_units(got, _composed(gpu_ctx, version, _stream_units(gpu_ctx, srcs, version, total=10 ** 9, cap=cap), total=10 ** 9, cap=cap), "cap")


# ------------------------------------------------------------------------------------------------------------------ files

def _file_units(ctx, files, version, **kw):
    """the files through the calls that existed: wav_decode / flac_decode and resample_streams, decode_streams"""
    units = []
    for j, b in enumerate(files):
        if b[:4] == b"DCSa":
            os_, s = D.dcsa_parse(b)
            one = {k: (None if v is None else [v[j]]) if k in ("budget", "cap") else v for k, v in kw.items()}
            units += _stream_units(ctx, [(s, os_)], version, **one)
        else:
            mono = (ctx.flac_decode if b[:4] == b"fLaC" else ctx.wav_decode)([b])[0]
            rate = 22050 if b[:4] == b"fLaC" else 44100
            units.append(("pcm", ctx.resample_streams([mono], rate)[0]))
    return units


def _files_call(ctx, files, version, **kw):
    return ctx.encode_files_budget(list(files), version, _fmt(version), **kw)


@pytest.mark.parametrize("order", ["listed", "reversed"])
@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_mixed_file_list(gpu_ctx, version, order):
    files = B.mixed_files(version) if order == "listed" else B.mixed_files(version)[::-1]
    units = _file_units(gpu_ctx, files, version)
    assert [u[0] for u in units] == (["pcm", "pcm", "pcm", "copy", "pcm"] if order == "listed" else ["pcm", "copy", "pcm", "pcm", "pcm"])
    budgets = B.rate_budgets(units, RATE)
    total = sum(budgets)
    for kw in (dict(budget=budgets), dict(total=total), dict()):
        got = _files_call(gpu_ctx, files, version, **kw)
        _check_units(got, _composed(gpu_ctx, version, units, **kw), (version, order, sorted(kw)))
        kinds = [int(k) for k in got[1]["kind"]]
        assert kinds == [D.FILE_DCSA_COPY if u[0] == "copy" else D.FILE_DCSA_REENCODE if f[:4] == b"DCSa" else D.FILE_FLAC if f[:4] == b"fLaC"
                         else D.FILE_WAV for u, f in zip(units, files)]
        assert [int(n) for n in got[1]["enc"]["nBytes"]] == [len(s) for s in got[0]]
        if order == "listed":
            key = "%x-%s" % (version, "shared" if "total" in kw else "per-job" if kw else "rate")
            assert B.digest(got[0], [B.info_of(r) for r in got[2]], got[-1] if "total" in kw else None) == GOLDEN["mixed"][key], key
    # the shared form really moves bytes: the near-silent file gives up its rate share, the dense one takes more than its own
    got = _files_call(gpu_ctx, files, version, total=total)
    quiet, dense = (4, 0) if order == "listed" else (0, 4)
    assert len(got[0][quiet]) < budgets[quiet] and len(got[0][dense]) > budgets[dense]
    assert int(got[3]["fits"]) == 1 and int(got[3]["usedBytes"]) == sum(len(s) for s in got[0]) <= total
    # reencode_all: the container of the target's family is searched too
    got = _files_call(gpu_ctx, files, version, reencode_all=True, total=total)
    _check_units(got, _composed(gpu_ctx, version, _file_units(gpu_ctx, files, version, reencode_all=True), total=total), "all")
    assert D.FILE_DCSA_COPY not in [int(k) for k in got[1]["kind"]]


@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_searched_containers_only_equal_existing_streams(gpu_ctx, version):
    srcs = _sources(0x7D0 + VERSIONS.index(version))[:4]
    files = [D.dcsa_header(os_, len(s)) + s for s, os_ in srcs]
    # (a container says OS94 for either 1994+ OS; the stream call is given what the container says)
    srcs = [(s, D.dcsa_parse(f)[0]) for (s, _), f in zip(srcs, files)]
    for kw in (dict(reencode_all=True, budget=[400, 500, 600, 700]), dict(reencode_all=True, total=2000), dict(total=10 ** 6)):
        got = _files_call(gpu_ctx, files, version, **kw)
        want = _stream_call(gpu_ctx, srcs, version, **kw)
        assert got[0] == want[0] and got[2].tobytes() == want[2].tobytes(), (version, sorted(kw))
        assert [int(a) for a in got[1]["enc"]["nBytes"]] == [int(a) for a in want[1]["enc"]["nBytes"]]
        if "total" in kw:
            assert got[3].tobytes() == want[3].tobytes()


@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_wav_only_equals_any_rate_pcm(gpu_ctx, version):
    files = [B.mixed_files(version)[0], B.mixed_files(version)[4]]
    mono = gpu_ctx.wav_decode(files)
    for kw in (dict(budget=[300, 40]), dict(total=350)):
        got = _files_call(gpu_ctx, files, version, **kw)
        want = gpu_ctx.encode_streams_at_budget(mono, 44100, version, _fmt(version), **kw)
        assert got[0] == want[0] and got[2].tobytes() == want[2].tobytes() and got[1]["enc"].tobytes() == want[1].tobytes()
        if "total" in kw:
            assert got[3].tobytes() == want[3].tobytes()


@pytest.mark.parametrize("version", VERSIONS, ids=IDS)
def test_damaged_container_in_the_middle(gpu_ctx, version):
    # (the damaged stream is a 1994+ one: searched under an OS93 target, and under 0x9400 where every container is)
    all_ = dict(reencode_all=True) if version == 0x9400 else {}
    files = list(B.mixed_files(version))
    good = _files_call(gpu_ctx, files, version, total=1200, **all_)
    bad = _bad_source()
    _, err, _ = gpu_ctx.decode_streams([(D.OS94, bad, 0x67, 0xFF)], extra_frames=1)
    assert err.any()
    files[1] = D.dcsa_header(D.OS94, len(bad)) + bad
    for kw in (dict(total=1200), dict(budget=[300] * 5)):
        with pytest.raises(D.DcsError) as e:
            _files_call(gpu_ctx, files, version, **kw, **all_)
        assert e.value.status == A.ERR_BAD_STREAM and "file 1: the decoder reports an error in a frame" in str(e.value)
    if version == 0x9400:
        # copied without a look inside, where the rule copies it
        assert _files_call(gpu_ctx, files, version, total=10 ** 6)[0][1] == bad
    again = _files_call(gpu_ctx, list(B.mixed_files(version)), version, total=1200, **all_)
    assert again[0] == good[0] and again[3].tobytes() == good[3].tobytes()


def test_refusals_say_what_is_wrong(gpu_ctx):
    x = np.zeros(480, np.float32)
    # an OS93 Type 1 target: the searched call's own message, under the budget call's name
    with pytest.raises(D.DcsError) as today:
        gpu_ctx.encode93_rd_streams([x], os_=D.OS93B, streamFormatType=1)
    tail = str(today.value).split("dcs_encode93_rd_streams", 1)[1]
    assert "Type 1 is not searched" in tail
    files = list(B.mixed_files(0x9302))
    srcs = _sources(0x7F0)[:2]
    for call, name in ((lambda: gpu_ctx.encode_streams_at_budget([x], 31250, 0x9302, D.FMT_93B_T1), "dcs_encode_streams_at_budget"),
                       (lambda: _stream_call_fmt(gpu_ctx, srcs, 0x9302, D.FMT_93B_T1), "dcs_transcode_streams_budget"),
                       (lambda: gpu_ctx.encode_files_budget(files, 0x9302, D.FMT_93B_T1), "dcs_encode_files_budget")):
        with pytest.raises(D.DcsError) as e:
            call()
        assert e.value.status == A.ERR_INVALID_ARG and str(e.value).endswith(name + tail), name
    # shared with budgetBytes set
    offs, out_offs = np.asarray([0, 480], np.uint64), np.zeros(2, np.uint64)
    rates, bud, out = np.asarray([31250], np.uint32), np.asarray([500], np.uint32), np.zeros(4096, np.uint8)
    p = D.transcode_params(0x9302)
    b = D.Budget(bud.ctypes.data, 900, None, 1, None)
    st = gpu_ctx.L.dcs_encode_streams_at_budget(gpu_ctx.h, x.ctypes.data, offs.ctypes.data, 1, rates.ctypes.data, None, None, 0, ctypes.byref(p),
                                                ctypes.byref(b), out.ctypes.data, out.size, out_offs.ctypes.data, None, None, None, 0, None)
    assert st == A.ERR_INVALID_ARG
    assert gpu_ctx.L.dcs_last_error(gpu_ctx.h).decode() == ("dcs_encode_streams_at_budget: budget->budgetBytes is for the per-job form; "
                                                           "the shared form takes totalBytes and capBytes")
    # a bad file is named by its place in the list, as dcs_encode_files names it
    for bad_file in (files[0][:30], b"fLaC" + bytes(40), b"neither of them"):
        with pytest.raises(D.DcsError) as want:
            gpu_ctx.encode_files([files[4], bad_file, files[0]], 0x9302)
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_files_budget([files[4], bad_file, files[0]], 0x9302, total=900)
        assert e.value.status == want.value.status and str(e.value) == str(want.value) and "file 1: " in str(e.value)
    # and the context still works
    assert len(gpu_ctx.encode_files_budget(files, 0x9302, total=1200)[0]) == 5


@pytest.mark.parametrize("version", [0x9400, 0x9302], ids=["9400", "9302"])
def test_budget_edges(gpu_ctx, version):
    files = B.mixed_files(version)
    units = _file_units(gpu_ctx, files, version)
    # a cap of 17 pins its job and reports fits = 0 for it alone
    cap = [10 ** 6, 10 ** 6, 17, 10 ** 6, 10 ** 6]
    got = _files_call(gpu_ctx, files, version, total=10 ** 6, cap=cap)
    assert [int(f) for f in got[2]["fits"]] == [1, 1, 0, 1, 1] and int(got[3]["fits"]) == 1
    _check_units(got, _composed(gpu_ctx, version, units, total=10 ** 6, cap=cap), "cap 17")
    # a total below the base reports fits = 0 for the call, and refuses nothing
    least = int(_files_call(gpu_ctx, files, version, total=10 ** 6)[3]["leastBytes"])
    got = _files_call(gpu_ctx, files, version, total=least - 1)
    assert int(got[3]["fits"]) == 0 and int(got[3]["usedBytes"]) == least == sum(len(s) for s in got[0])
    _check_units(got, _composed(gpu_ctx, version, units, total=least - 1), "under")


@pytest.mark.parametrize("version", [0x9400, 0x9302], ids=["9400", "9302"])
def test_several_groups_write_the_one_group_bytes(gpu_ctx, dcs, version):
    files = B.mixed_files(version)
    total = sum(B.rate_budgets(_file_units(gpu_ctx, files, version), RATE))
    one = _files_call(gpu_ctx, files, version, total=total)
    srcs = _sources(0x7E0)
    one_s = _stream_call(gpu_ctx, srcs, version, total=3000, reencode_all=True)
    try:
        for cap in (1, 35):
            dcs.encode_sweep_group_frames(cap)
            got = _files_call(gpu_ctx, files, version, total=total)
            assert got[0] == one[0] and got[2].tobytes() == one[2].tobytes() and got[3].tobytes() == one[3].tobytes(), cap
            got = _stream_call(gpu_ctx, srcs, version, total=3000, reencode_all=True)
            assert got[0] == one_s[0] and got[3].tobytes() == one_s[3].tobytes(), cap
    finally:
        dcs.encode_sweep_group_frames(0)


@pytest.mark.parametrize("shared", [False, True], ids=["per-job", "shared"])
def test_capacity_one_byte_short(gpu_ctx, shared):
    version = 0x9400
    files = list(B.mixed_files(version))
    kw = dict(total=1200) if shared else dict(budget=[300, 200, 300, 400, 100])
    full = _files_call(gpu_ctx, files, version, **kw)
    size = sum(len(s) for s in full[0])
    blob = np.frombuffer(b"".join(files), np.uint8)
    offs = np.cumsum([0] + [len(f) for f in files]).astype(np.uint64)
    p = D.transcode_params(version, _fmt(version))
    bud = np.asarray(kw.get("budget", [0] * 5), np.uint32)
    fit = np.zeros(1, D.ENCODE_RD_FIT_INFO_DTYPE)
    b = D.Budget(bud.ctypes.data if not shared else None, kw.get("total", 0), None, int(shared), fit.ctypes.data)
    out, out_offs = np.zeros(size, np.uint8), np.zeros(6, np.uint64)
    info, info_rd = np.zeros(5, D.ENCODE_FILE_INFO_DTYPE), np.zeros(5, D.ENCODE_RD_INFO_DTYPE)
    args = lambda room: (gpu_ctx.h, blob.ctypes.data, offs.ctypes.data, 5, ctypes.byref(p), None, 0, ctypes.byref(b), out.ctypes.data, room,
                         out_offs.ctypes.data, info.ctypes.data, info_rd.ctypes.data, None, 0, None)
    assert gpu_ctx.L.dcs_encode_files_budget(*args(size - 1)) == A.ERR_CAPACITY
    assert not out.any() and [int(v) for v in np.diff(out_offs)] == [len(s) for s in full[0]]
    if shared:
        # (the record as the allocator leaves it: sqErr is summed once the streams are written)
        assert FR.record_tuple(fit[0])[:3] + FR.record_tuple(fit[0])[4:] == FR.record_tuple(full[3])[:3] + FR.record_tuple(full[3])[4:]
    else:
        assert info_rd.tobytes() == full[2].tobytes() and info.tobytes() == full[1].tobytes()
    assert gpu_ctx.L.dcs_encode_files_budget(*args(size)) == 0
    assert out.tobytes() == b"".join(full[0]) and info_rd.tobytes() == full[2].tobytes()
