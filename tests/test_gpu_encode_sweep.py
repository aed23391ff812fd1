"""dcs_encode_sweep and Context.encode_fit on the MI355X: every job's bytes are the one-set entry point's (hence the
reference's), job lists in any order, the round-trip sums integer for integer those of the restatement over the oracle's
decode (tests/sweep_ref.py) and those recorded from the compiled reference (tests/golden/sweep_golden.json), the fit end to
end against the CPU restatements, the grouped path, and loud errors."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc_ref as E
import enc93_ref as R
import sweep_ref as S
from dcsexplorer_amd.api import EncodeParams, _encode_input, _ptr
from test_gpu_encode import _signal

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ARR = np.load(os.path.join(HERE, "golden", "encode_golden.npz"))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "sweep_golden.json")))["cases"]
F32 = lambda v: float(np.float32(v))        # noqa: E731

# five sets that differ in every field and mix fixed layouts with wildcards: (fmt, (type, sub-type) for enc_ref, params)
SETS94 = [
    (None, (-1, -1), dict(powerBandCutoff=F32(0.97), targetBitRate=128000, minimumDynamicRange=F32(10 / 32768), maximumQuantizationError=F32(10 / 32768))),
    (D.FMT_94_T1_S3, (1, 3), dict(powerBandCutoff=F32(0.9), targetBitRate=48000, minimumDynamicRange=F32(2 / 32768), maximumQuantizationError=F32(30 / 32768))),
    (D.FMT_94_T0, (0, 0), dict(powerBandCutoff=F32(0.995), targetBitRate=192000, minimumDynamicRange=F32(0), maximumQuantizationError=F32(6 / 32768))),
    (None, (-1, -1), dict(powerBandCutoff=F32(1.0), targetBitRate=320000, minimumDynamicRange=F32(40 / 32768), maximumQuantizationError=F32(2 / 32768))),
    (D.FMT_94_T1_S0, (1, 0), dict(powerBandCutoff=F32(0.8), targetBitRate=24000, minimumDynamicRange=F32(4 / 32768), maximumQuantizationError=F32(16 / 32768))),
]
SETS93 = {
    D.OS93B: [(None, -1, SETS94[0][2]), (D.FMT_93B_T1, 1, SETS94[1][2]), (D.FMT_93_T0, 0, SETS94[2][2]), (None, -1, SETS94[3][2]),
              (D.FMT_93B_T1, 1, SETS94[4][2])],
    D.OS93A: [(None, -1, SETS94[0][2]), (D.FMT_93_T0, 0, SETS94[1][2]), (D.FMT_93_T0, 0, SETS94[2][2]), (None, -1, SETS94[3][2]),
              (None, -1, SETS94[4][2])],
}


def _batch(seed):
    rng = np.random.default_rng(0x5EEB + seed)
    lengths = [1, 2, 239, 240, 241, 479, 481] + [int(np.exp(rng.uniform(np.log(240), np.log(240 * 600)))) for _ in range(20)]
    lengths.append(int(rng.integers(240 * 2000, 240 * 3000)))
    return [_signal(rng, n) for n in lengths]


def _same(a, b):
    """two SWEEP_RESULT_DTYPE arrays field by field (their padding bytes are nobody's)"""
    return a.shape == b.shape and bool((a == b).all())


def _same_info(a, b):
    return all(a[k] == b[k] for k in ("formatType", "formatSubType", "nFrames", "nBytes", "bandsToKeep"))


def test_bytes_equal_the_one_set_entry_point_and_enc_ref(gpu_ctx):
    pcm = _batch(0)
    sets = [D.encode_params(fmt, **p) for fmt, _, p in SETS94]
    streams, res = gpu_ctx.encode_sweep(pcm, sets, measure=False)
    assert len(streams) == len(pcm) * len(sets) and not res["measured"].any()
    for k, (fmt, ref_fmt, p) in enumerate(SETS94):
        for i, x in enumerate(pcm):
            alone, info = gpu_ctx.encode_streams([x], fmt, **p)
            j = i * len(sets) + k
            assert streams[j] == alone[0], (i, k)
            assert _same_info(res["enc"][j], info[0]), (i, k)
            if (i + k) % 5 == 0 and len(x) < 240 * 700:
                want, win, keep = E.encode(x, ref_fmt, **p)
                assert streams[j] == want and (res["enc"][j]["formatType"], res["enc"][j]["formatSubType"]) == win


@pytest.mark.parametrize("os_", [D.OS93B, D.OS93A])
def test_os93_bytes_equal_encode93_streams(gpu_ctx, os_):
    pcm = _batch(1)[:20] + _batch(1)[-1:]
    version = 0x9302 if os_ == D.OS93B else 0x9301
    sets = [D.encode93_params(os_, fmt, **p) for fmt, _, p in SETS93[os_]]
    streams, res = gpu_ctx.encode_sweep(pcm, sets, measure=False)
    for k, (fmt, typ, p) in enumerate(SETS93[os_]):
        for i, x in enumerate(pcm):
            alone, info = gpu_ctx.encode93_streams([x], os_, fmt, **p)
            j = i * len(sets) + k
            assert streams[j] == alone[0], (i, k)
            assert _same_info(res["enc"][j], info[0]), (i, k)
            if (i + k) % 7 == 0 and len(x) < 240 * 700:
                assert streams[j] == R.encode(x, version, typ, **p)[0]


def test_job_lists(gpu_ctx):
    pcm = _batch(2)[:18]
    sets = [D.encode_params(fmt, **p) for fmt, _, p in SETS94]
    n, k = len(pcm), len(sets)
    every, res = gpu_ctx.encode_sweep(pcm, sets)
    pairs = [(i, r) for i in range(n) for r in range(k)]
    listed, res_l = gpu_ctx.encode_sweep(pcm, sets, pairs)
    assert listed == every and _same(res_l, res)
    order = np.random.default_rng(7).permutation(n * k)
    shuffled, res_s = gpu_ctx.encode_sweep(pcm, sets, [pairs[j] for j in order])
    assert shuffled == [every[j] for j in order] and _same(res_s, res[order])
    # one job per stream, each with a set of its own: per-stream parameters
    per = [(i, (3 * i + 1) % k) for i in range(n)]
    own, res_o = gpu_ctx.encode_sweep(pcm, sets, per)
    assert own == [every[i * k + r] for i, r in per] and _same(res_o, res[[i * k + r for i, r in per]])
    # the same pair twice
    twice, res_t = gpu_ctx.encode_sweep(pcm, sets, [(4, 2), (0, 0), (4, 2)])
    assert twice == [every[4 * k + 2], every[0], every[4 * k + 2]] and res_t[0] == res_t[2] == res[4 * k + 2]
    # no bytes asked for: the same records
    none, res_n = gpu_ctx.encode_sweep(pcm, sets, streams=False)
    assert none is None and _same(res_n, res)
    # a job does not depend on what else is in the batch
    few, res_f = gpu_ctx.encode_sweep(pcm[5:9][::-1], sets[1:3])
    assert few == [every[i * k + r] for i in (8, 7, 6, 5) for r in (1, 2)]
    assert _same(res_f, res[[i * k + r for i in (8, 7, 6, 5) for r in (1, 2)]])
    # an empty job list
    nothing, res_e = gpu_ctx.encode_sweep(pcm, sets, [])
    assert nothing == [] and len(res_e) == 0


def test_groups_give_the_same_results(gpu_ctx):
    """the grouped path (what an allocation failure leads to), forced by a cap on a group's job-frames"""
    pcm = _batch(3)[:16]
    sets = [D.encode_params(fmt, **p) for fmt, _, p in SETS94[:3]]
    whole, res = gpu_ctx.encode_sweep(pcm, sets)
    alone, _ = gpu_ctx.encode_streams(pcm)
    try:
        for cap in (1, 700, 5000):
            D.encode_sweep_group_frames(cap)
            parts, res_p = gpu_ctx.encode_sweep(pcm, sets)
            assert parts == whole and _same(res_p, res), cap
            none, res_n = gpu_ctx.encode_sweep(pcm, sets, streams=False)
            assert none is None and _same(res_n, res), cap
            assert gpu_ctx.encode_streams(pcm)[0] == alone
    finally:
        D.encode_sweep_group_frames(0)


def _want(oracle, x, stream, os_):
    n_frames = (stream[0] << 8) | stream[1]
    return S.measure(x, oracle.decode(os_, 255, [stream], [255], n_frames + 1))


def _check_measured(r, want, what):
    assert r["measured"] == 1, what
    got = {k: int(r[k]) for k in ("nCompared", "sumSrcSq", "sumDecSq", "sumCross", "peakErr")}
    assert got == want, what


def test_measurement_is_exact(gpu_ctx, oracle):
    rng = np.random.default_rng(0x3EA5)
    pcm = [ARR[k + "/pcm"] for k in ("len1", "silence", "dc", "square", "noise_fs", "rec0", "float_tones", "len239", "len241")]
    pcm += [np.array([0.25], np.float32), np.zeros(1, np.int16), np.array([1.0, -1.0] * 300, np.float32)]
    pcm += [_signal(rng, int(rng.integers(1, 240 * 120))) for _ in range(12)]
    sets = [D.encode_params(fmt, **p) for fmt, _, p in SETS94]
    streams, res = gpu_ctx.encode_sweep(pcm, sets)
    for j, (s, r) in enumerate(zip(streams, res)):
        x = pcm[j // len(sets)]
        _check_measured(r, _want(oracle, x, s, D.OS95 if r["enc"]["formatSubType"] == 3 else D.OS94), j)
    assert int(res[1 * len(sets)]["sumSrcSq"]) == 0                       # silence
    assert max(int(r["peakErr"]) for r in res[3 * len(sets):5 * len(sets)]) > 0     # square, noise_fs: clipping on both sides
    for os_ in (D.OS93B, D.OS93A):
        sets93 = [D.encode93_params(os_, fmt, **p) for fmt, _, p in SETS93[os_]]
        streams, res = gpu_ctx.encode_sweep(pcm[:14], sets93)
        unread = 0
        for j, (s, r) in enumerate(zip(streams, res)):
            if os_ == D.OS93A and r["enc"]["bandsToKeep"] == 0:
                # sixteen 0xFF header bytes: the type bit is set, and every decoder reads OS93a Type 1 with 31 bands
                assert s[2:18] == b"\xff" * 16 and r["measured"] == 0 and D.sweep_sq_err(r) == [0] and r["nCompared"] == 0
                unread += 1
                continue
            _check_measured(r, _want(oracle, pcm[j // len(sets93)], s, os_), (os_, j))
        assert (unread > 0) == (os_ == D.OS93A)


def test_measurement_equals_the_compiled_reference(gpu_ctx):
    pcm = [ARR["rec%d/pcm" % v] for v in range(4)]
    sets = [D.encode_params(None, targetBitRate=r) for r in S.RATES]
    streams, res = gpu_ctx.encode_sweep(pcm, sets)
    assert len(GOLDEN) == len(streams) == 24
    for j, (c, s, r) in enumerate(zip(GOLDEN, streams, res)):
        assert (c["signal"], c["targetBitRate"]) == ("rec%d" % (j // 6), S.RATES[j % 6])
        assert len(s) == c["bytes"] and hashlib.sha256(s).hexdigest() == c["sha256"]
        assert [r["enc"]["formatType"], r["enc"]["formatSubType"]] == c["winner"]
        _check_measured(r, {k: c[k] for k in ("nCompared", "sumSrcSq", "sumDecSq", "sumCross", "peakErr")}, c["signal"])
    assert D.sweep_sq_err(res) == [c["sqErrAtLag"][S.LAG] for c in GOLDEN]


def test_a_long_stream_measures_the_same(gpu_ctx, oracle):
    """one long stream that dominates the list is decoded through the host-planned batch, as transcoding does it"""
    rng = np.random.default_rng(0x10A6)
    pcm = [_signal(rng, 240 * 2600 + 5), _signal(rng, 240 * 3)]
    sets = [D.encode_params(None), D.encode_params(D.FMT_94_T1_S3, targetBitRate=64000)]
    streams, res = gpu_ctx.encode_sweep(pcm, sets)
    for j, (s, r) in enumerate(zip(streams, res)):
        assert s == gpu_ctx.encode_streams([pcm[j // 2]], [None, D.FMT_94_T1_S3][j % 2], targetBitRate=[128000, 64000][j % 2])[0][0]
        _check_measured(r, _want(oracle, pcm[j // 2], s, D.OS95 if r["enc"]["formatSubType"] == 3 else D.OS94), j)


def fit_inputs():
    """the 16 streams of the end-to-end case: the four golden recordings and 12 seeded signals"""
    rng = np.random.default_rng(0x5EE9)
    lengths = rng.integers(240 * 20, 240 * 200, 12)
    return [ARR["rec%d/pcm" % v] for v in range(4)] + [_signal(rng, int(n)) for n in lengths]


def cpu_tables(oracle, pcm):
    """sizes, squared errors and streams [stream][rate] from the CPU restatements: enc_ref for the bytes, the oracle for the decode"""
    n_bytes, sq_err, streams = [], [], []
    for x in pcm:
        row = [E.encode(x, (-1, -1), targetBitRate=r) for r in S.RATES]
        streams.append([s for s, _, _ in row])
        n_bytes.append([len(s) for s, _, _ in row])
        sq_err.append([S.sq_err(_want(oracle, x, s, D.OS95 if win[1] == 3 else D.OS94)) for s, win, _ in row])
    return n_bytes, sq_err, streams


def test_fit_end_to_end(gpu_ctx, oracle):
    pcm = fit_inputs()
    n_bytes, sq_err, ref_streams = cpu_tables(oracle, pcm)
    totals = [sum(row[r] for row in n_bytes) for r in range(len(S.RATES))]
    assert all(a > b for a, b in zip(totals, totals[1:])), totals
    sets = [D.encode_params(None, targetBitRate=r) for r in S.RATES]
    for lo in (1, 3):
        budget = (totals[lo] + totals[lo + 1]) // 2
        status, choice, total = S.fit(n_bytes, sq_err, budget)
        assert status == 0
        streams, got_choice, res, got_total = gpu_ctx.encode_fit(pcm, sets, budget)
        assert got_choice.tolist() == choice and got_total == total <= budget
        assert sum(len(s) for s in streams) == total
        for i, s in enumerate(streams):
            assert s == ref_streams[i][choice[i]], i
            assert int(res[i]["enc"]["nBytes"]) == len(s) and D.sweep_sq_err(res[i])[0] == sq_err[i][choice[i]]
    with pytest.raises(D.DcsError) as e:
        gpu_ctx.encode_fit(pcm, sets, 1)
    assert e.value.status == -5 and e.value.needed == min(totals) and str(min(totals)) in str(e.value)


def _raw_sweep(ctx, pcm_list, sets, jobs, flags, cap, want_results=True):
    x, offs = _encode_input(pcm_list)
    arr = (EncodeParams * max(len(sets), 1))(*sets)
    n_jobs = len(jobs) if jobs is not None else len(pcm_list) * len(sets)
    jl = None
    if jobs is not None:
        jl = np.array(jobs, dtype=np.uint32).reshape(-1, 2).view(D.SWEEP_JOB_DTYPE).reshape(-1) if jobs else np.zeros(1, D.SWEEP_JOB_DTYPE)
    res = np.zeros(max(n_jobs, 1), D.SWEEP_RESULT_DTYPE)
    out_offs = np.zeros(n_jobs + 1, np.uint64)
    out = np.zeros(max(cap, 1), np.uint8)
    st = ctx.L.dcs_encode_sweep(ctx.h, _ptr(x), _ptr(offs), len(pcm_list), arr if sets else None, len(sets),
                                _ptr(jl) if jl is not None else None, n_jobs, flags, _ptr(res) if want_results else None,
                                _ptr(out) if cap else None, cap, _ptr(out_offs))
    msg = ctx.L.dcs_last_error(ctx.h)
    return st, out_offs, res, (msg.decode() if msg else "")


def test_error_paths(gpu_ctx):
    ok = np.zeros(480, np.float32)
    p94, p93b, p93a = D.encode_params(), D.encode93_params(D.OS93B), D.encode93_params(D.OS93A)
    for sets in ([p94, p93b], [p93b, p93a], [p93a, p94]):                   # mixed families
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_sweep([ok], sets)
        assert e.value.status == -1 and "one encoder" in str(e.value)
    for sets in ([p94, D.encode_params(targetBitRate=0)], [D.encode_params(streamFormatSubType=1)],
                 [p93a, D.encode93_params(D.OS93A, streamFormatType=1)]):   # a set its encoder refuses
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_sweep([ok], sets)
        assert e.value.status == -1
    for jobs in ([(0, 0), (2, 0)], [(0, 2)]):                               # a job out of range
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_sweep([ok, ok], [p94, p94], jobs)
        assert e.value.status == -1 and "job %d" % (len(jobs) - 1) in str(e.value)
    assert _raw_sweep(gpu_ctx, [ok], [], None, 0, 0)[0] == -1                # nSets == 0
    assert _raw_sweep(gpu_ctx, [ok], [p94], None, 2, 0)[0] == -1             # an unknown flag
    assert _raw_sweep(gpu_ctx, [ok], [p94], None, D.SWEEP_MEASURE, 0, want_results=False)[0] == -1
    for bad, status, word in [([ok, np.array([0.1, np.nan], np.float32)], -6, "stream 1"), ([np.array([0.5, 1.0001], np.float32), ok], -6, "stream 0"),
                              ([ok, np.zeros(0, np.float32)], -1, "stream 1: empty"),
                              ([np.zeros(65535 * 240 + 1, np.float32)], -1, "more than 65 535 frames")]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_sweep(bad, [p94, p94])
        assert e.value.status == status and word in str(e.value)
    # capacity: refused with every offset filled; sizes only (no buffer at all) is DCS_OK with the same offsets
    want, _ = gpu_ctx.encode_sweep([ok, ok], [p94, D.encode_params(targetBitRate=48000)], measure=False)
    st, offs, res, _ = _raw_sweep(gpu_ctx, [ok, ok], [p94, D.encode_params(targetBitRate=48000)], None, 0, 8)
    assert st == -5 and np.diff(offs.astype(np.int64)).tolist() == [len(s) for s in want]
    st, offs0, res0, _ = _raw_sweep(gpu_ctx, [ok, ok], [p94, D.encode_params(targetBitRate=48000)], None, 0, 0)
    assert st == 0 and offs0.tolist() == offs.tolist() and _same(res0, res)
    # a stream of 65 535 frames encodes, but cannot be measured: the extra frame would be the 65 536th
    full = np.zeros(65535 * 240, np.float32)
    streams, res = gpu_ctx.encode_sweep([full], [p94], measure=False)
    assert res[0]["enc"]["nFrames"] == 65535 and streams[0][:2] == b"\xff\xff"
    with pytest.raises(D.DcsError) as e:
        gpu_ctx.encode_sweep([ok, full], [p94])
    assert e.value.status == -1 and "stream 1" in str(e.value) and "65 535" in str(e.value)
