"""dcs_encode93a_sweep, Context.encode93a_fit and the plain Type-1 call through the one driver, on the MI355X.  Expected
bytes and info records come from the numpy restatement (tests/enc93a_ref.py through tests/enc93a_cases.py), Type-0 jobs
from encode93_streams, the measured sums from tests/sweep_ref.py over the library's existing decoder's PCM of the RESTATED
bytes; nothing expected comes from the call under test."""
import hashlib
import json

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc93a_cases as C
import enc93a_ref as A
import enc93a_sweep_cases as L
import sweep_ref as S
from dcsexplorer_amd.api import EncodeParams, _encode_input, _ptr

pytestmark = pytest.mark.gpu

PCM = [C.SIGNALS[n] for n in C.NAMES]
# {4 rates} x {2 q} Type 1, and one Type-0 set among them (set 3)
T1 = [(rate, mqe) for rate in C.RATES for mqe in C.MQES]
T0_AT = 3
SETS = [D.encode93a_params(D.FMT_93A_T1, **C.params(rate, mqe)) for rate, mqe in T1]
SETS.insert(T0_AT, D.encode93a_params(D.FMT_93_T0))
K = len(SETS)
SUMS = ("nCompared", "sumSrcSq", "sumDecSq", "sumCross", "peakErr")


def t1_of(r):
    """set r of SETS -> its (rate, mqe), or None for the Type-0 set"""
    return None if r == T0_AT else T1[r if r < T0_AT else r - 1]


def _same(a, b):
    return a.shape == b.shape and bool((a == b).all())


@pytest.fixture(scope="module")
def every(gpu_ctx):
    """every pair, stream-major, measured: (bytes, results, info93a)"""
    return gpu_ctx.encode93a_sweep(PCM, SETS)


@pytest.fixture(scope="module")
def decoded(gpu_ctx):
    """the RESTATED Type-1 stream of every (signal, Type-1 set), decoded by the library's decoder with one extra frame:
    {(name, rate, mqe): int16 [nFrames + 1, 240]}"""
    keys = [(name, rate, mqe) for name in C.NAMES for rate, mqe in T1]
    pcm, err, first = gpu_ctx.decode_streams([(D.OS93A, C.type1(*k)[0], 255, 0xFF) for k in keys], extra_frames=1)
    assert not err.any()
    return {k: pcm[first[i]:first[i + 1]] for i, k in enumerate(keys)}


def test_every_pair_equals_the_restatement(gpu_ctx, every):
    streams, res, infa = every
    assert len(streams) == len(PCM) * K == len(res) == len(infa)
    t0, t0_info = gpu_ctx.encode93_streams(PCM, D.OS93A, D.FMT_93_T0)
    for i, name in enumerate(C.NAMES):
        for r in range(K):
            j, e = i * K + r, res["enc"][i * K + r]
            if t1_of(r) is None:
                assert streams[j] == t0[i] and e == t0_info[i], (name, r)
                assert not any(int(infa[j][k]) for k in L.INFO_KEYS), (name, r)
                continue
            s, typ, keep, ch = C.expected(name, *t1_of(r), 1)
            assert streams[j] == s, (name, r)
            assert (e["formatType"], e["formatSubType"], e["nFrames"], e["nBytes"], e["bandsToKeep"]) == (1, 0, (s[0] << 8) | s[1], len(s), keep)
            assert [int(infa[j][k]) for k in L.INFO_KEYS] == [ch[k] for k in L.INFO_KEYS], (name, r)
            assert s[2] == 0x80 | ch["selector"] << 5 | ch["numBands"]
    assert min(len(s) for s in streams) == 4                 # the shortest stream there is: 3 header bytes and a terminator


def test_job_lists(gpu_ctx, every):
    streams, res, infa = every
    n = len(PCM)
    pairs = [(i, r) for i in range(n) for r in range(K)]
    rng = np.random.default_rng(0x93A5)
    order = [int(j) for j in rng.permutation(n * K)[:40]] + [5, 5, 17]                  # shuffled, with repeats
    got, res_g, infa_g = gpu_ctx.encode93a_sweep(PCM, SETS, [pairs[j] for j in order])
    assert got == [streams[j] for j in order] and _same(res_g, res[order]) and _same(infa_g, infa[order])
    # stream 0 only under q = MQES[0], stream 1 only under MQES[1], stream 2 under both, stream 3 in no Type-1 job at all
    q0 = [r for r in range(K) if t1_of(r) and t1_of(r)[1] == C.MQES[0]]
    q1 = [r for r in range(K) if t1_of(r) and t1_of(r)[1] == C.MQES[1]]
    jobs = [(1, q1[0]), (0, q0[1]), (2, q1[2]), (0, q0[3]), (3, T0_AT), (2, q0[0]), (1, q1[3])]
    got, res_g, infa_g = gpu_ctx.encode93a_sweep(PCM, SETS, jobs)
    at = [i * K + r for i, r in jobs]
    assert got == [streams[j] for j in at] and _same(res_g, res[at]) and _same(infa_g, infa[at])
    # one job per stream: per-stream parameters
    per = [(i, (5 * i + 2) % K) for i in range(n)]
    got, res_g, infa_g = gpu_ctx.encode93a_sweep(PCM, SETS, per)
    at = [i * K + r for i, r in per]
    assert got == [streams[j] for j in at] and _same(res_g, res[at]) and _same(infa_g, infa[at])
    # a job does not depend on what else is in the call: other streams, other sets, other distinct q
    few = [SETS[6], SETS[T0_AT], SETS[1]]
    got, res_g, infa_g = gpu_ctx.encode93a_sweep(PCM[4:7][::-1], few)
    at = [i * K + r for i in (6, 5, 4) for r in (6, T0_AT, 1)]
    assert got == [streams[j] for j in at] and _same(res_g, res[at]) and _same(infa_g, infa[at])
    nothing, res_e, _ = gpu_ctx.encode93a_sweep(PCM, SETS, [])
    assert nothing == [] and len(res_e) == 0


def test_more_distinct_q_than_a_launch_walks(gpu_ctx, every):
    """eleven distinct maximumQuantizationError values: A1 is launched twice; the two known ones keep their results"""
    streams, res, infa = every
    extra = [float(np.float32(v / 32768)) for v in (1, 2, 3, 4, 5, 6, 7, 8, 9)]
    sets = [D.encode93a_params(D.FMT_93A_T1, targetBitRate=64000, maximumQuantizationError=q) for q in [C.MQES[0]] + extra + [C.MQES[1]]]
    got, res_g, infa_g = gpu_ctx.encode93a_sweep(PCM, sets, measure=False)
    k = len(sets)
    for i, name in enumerate(C.NAMES):
        for r, mqe in ((0, C.MQES[0]), (k - 1, C.MQES[1])):
            s, _, _, ch = C.expected(name, 64000, mqe, 1)
            assert got[i * k + r] == s and [int(infa_g[i * k + r][key]) for key in L.INFO_KEYS] == [ch[key] for key in L.INFO_KEYS]
    # the floors in between are a restatement away: one signal, every q
    an = C.analysis("noise_m60")
    i = C.NAMES.index("noise_m60")
    for r, q in enumerate(extra, 1):
        assert got[i * k + r] == A.encode_type1(an, targetBitRate=64000, maximumQuantizationError=q)[0], q


def test_groups_give_the_same_results(gpu_ctx, every):
    streams, res, infa = every
    rs = [2, T0_AT, 7, 1]
    sets = [SETS[r] for r in rs]
    at = [i * K + r for i in range(len(PCM)) for r in rs]
    longest = max((len(x) + 239) // 240 for x in PCM)
    assert longest == 6 and sum((len(x) + 239) // 240 == longest for x in PCM) > 1       # such a stream's jobs: a group each
    try:
        D.encode_sweep_group_frames(longest)
        got, res_g, infa_g = gpu_ctx.encode93a_sweep(PCM, sets)
        assert got == [streams[j] for j in at] and _same(res_g, res[at]) and _same(infa_g, infa[at])
        got, res_u, infa_u = gpu_ctx.encode93a_sweep(PCM, sets, measure=False)
        assert got == [streams[j] for j in at] and _same(res_u["enc"], res["enc"][at]) and not res_u["measured"].any()
        assert _same(infa_u, infa[at])
        none, res_n, _ = gpu_ctx.encode93a_sweep(PCM, sets, streams=False)
        assert none is None and _same(res_n, res[at])
    finally:
        D.encode_sweep_group_frames(0)


def test_the_plain_call_under_a_group_cap(gpu_ctx):
    whole = gpu_ctx.encode93a_streams(PCM, D.FMT_93A_T1, targetBitRate=64000)
    wild = gpu_ctx.encode93a_streams(PCM, None, targetBitRate=64000)
    try:
        for cap in (1, 6, 11):
            D.encode_sweep_group_frames(cap)
            for want, fmt in ((whole, D.FMT_93A_T1), (wild, None)):
                got = gpu_ctx.encode93a_streams(PCM, fmt, targetBitRate=64000)
                assert got[0] == want[0] and _same(got[1], want[1]) and _same(got[2], want[2]), cap
    finally:
        D.encode_sweep_group_frames(0)
    for i, name in enumerate(C.NAMES):
        assert whole[0][i] == C.type1(name, 64000, A.DEFAULTS["maximumQuantizationError"])[0]


def test_every_type1_job_is_measured_exactly(gpu_ctx, every, decoded):
    streams, res, infa = every
    for i, name in enumerate(C.NAMES):
        for r in range(K):
            if t1_of(r) is None:
                continue
            rec = res[i * K + r]
            assert rec["measured"] == 1, (name, r)
            want = S.measure(C.SIGNALS[name], decoded[(name,) + t1_of(r)])
            assert {k: int(rec[k]) for k in SUMS} == want, (name, r)
    # the Type-0 jobs: the records of the OS93 sweep for the same set
    t0, res0 = gpu_ctx.encode_sweep(PCM, [D.encode93_params(D.OS93A, D.FMT_93_T0)])
    assert _same(res[T0_AT::K], res0) and (res0["measured"] == 1).any()
    assert any(int(r["peakErr"]) > 0 for r in res) and int(res[C.NAMES.index("silence") * K]["sumSrcSq"]) == 0


def test_the_decoder_under_the_sums_is_the_references(reference, decoded):
    names = [n for n in C.NAMES if n.startswith("rec:")] + ["noise_fs"]
    assert len(names) > 2
    for name in names:
        for rate, mqe in T1:
            s = C.type1(name, rate, mqe)[0]
            want = reference.decode(D.OS93A, 255, [s], [0xFF], ((s[0] << 8) | s[1]) + 1)
            assert np.array_equal(decoded[(name, rate, mqe)], want), (name, rate, mqe)


def test_a_long_stream_is_measured_through_the_host_planned_batch(gpu_ctx):
    """2 049 frames alone in the call: more than 2 048, and 64 times that is more than the call's job-frames"""
    golden = json.load(open(L.GOLDEN))["cases"]
    assert [c["targetBitRate"] for c in golden] == L.LONG_RATES
    x = L.long_signal()
    sets = [D.encode93a_params(D.FMT_93A_T1, targetBitRate=r) for r in L.LONG_RATES]
    streams, res, infa = gpu_ctx.encode93a_sweep([x], sets)
    for j, c in enumerate(golden):
        s = streams[j]
        assert (s[0] << 8 | s[1], len(s), hashlib.sha256(s).hexdigest()) == (L.LONG_FRAMES, c["nBytes"], c["sha256"]), c["targetBitRate"]
        assert {k: int(infa[j][k]) for k in L.INFO_KEYS} == c["info"]
        # (the bytes are the restated ones, by their hash: decoded by the existing decoder for the expected sums)
        pcm, err, _ = gpu_ctx.decode_streams([(D.OS93A, s, 255, 0xFF)], extra_frames=1)
        assert not err.any() and res[j]["measured"] == 1
        assert {k: int(res[j][k]) for k in SUMS} == S.measure(x, pcm), c["targetBitRate"]
    unmeasured, res_u, infa_u = gpu_ctx.encode93a_sweep([x], sets, measure=False)
    assert unmeasured == streams and _same(infa_u, infa)


def _raw(ctx, pcm_list, sets, jobs, flags, cap):
    x, offs = _encode_input(pcm_list)
    arr = (EncodeParams * len(sets))(*sets)
    n_jobs = len(jobs) if jobs is not None else len(pcm_list) * len(sets)
    jl = np.array(jobs, dtype=np.uint32).reshape(-1, 2).view(D.SWEEP_JOB_DTYPE).reshape(-1) if jobs else None
    res, infa = np.zeros(max(n_jobs, 1), D.SWEEP_RESULT_DTYPE), np.zeros(max(n_jobs, 1), D.ENCODE93A_INFO_DTYPE)
    out_offs = np.zeros(n_jobs + 1, np.uint64)
    out = np.zeros(max(cap, 1), np.uint8)
    st = ctx.L.dcs_encode93a_sweep(ctx.h, _ptr(x), _ptr(offs), len(pcm_list), arr, len(sets), _ptr(jl) if jl is not None else None, n_jobs,
                                   flags, _ptr(res), _ptr(infa), _ptr(out) if cap else None, cap, _ptr(out_offs))
    return st, out_offs, res, infa, out


def test_sizes_only_capacity_and_errors(gpu_ctx, every):
    streams, res, infa = every
    none, res_n, infa_n = gpu_ctx.encode93a_sweep(PCM, SETS, streams=False)
    assert none is None and _same(res_n, res) and _same(infa_n, infa)
    none, res_n, infa_n = gpu_ctx.encode93a_sweep(PCM, SETS, measure=False, streams=False)
    assert _same(res_n["enc"], res["enc"]) and not res_n["measured"].any() and _same(infa_n, infa)
    # a short buffer: -5, every offset filled, nothing written
    st, offs, res_c, infa_c, out = _raw(gpu_ctx, PCM, SETS, None, 0, 8)
    assert st == -5 and np.diff(offs.astype(np.int64)).tolist() == [len(s) for s in streams] and not out.any()
    assert _same(res_c["enc"], res["enc"]) and _same(infa_c, infa)
    ok = np.zeros(480, np.float32)
    t1, t0 = D.encode93a_params(D.FMT_93A_T1), D.encode93a_params(D.FMT_93_T0)
    for bad in (D.encode93a_params(None), D.encode93_params(D.OS93B), D.encode_params(), D.encode93a_params(D.FMT_93A_T1, targetBitRate=0)):
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode93a_sweep([ok], [t1, t0, bad])
        assert e.value.status == -1 and "set 2" in str(e.value)
    for jobs in ([(0, 0), (2, 0)], [(0, 2)]):
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode93a_sweep([ok, ok], [t1, t0], jobs)
        assert e.value.status == -1 and "job %d" % (len(jobs) - 1) in str(e.value)
    for pcm, status, word in [([ok, np.array([0.1, np.nan], np.float32)], -6, "stream 1"), ([np.array([0.5, 1.0001], np.float32), ok], -6, "stream 0"),
                              ([ok, np.zeros(0, np.float32)], -1, "stream 1: empty"),
                              ([np.zeros(65535 * 240 + 1, np.float32)], -1, "more than 65 535 frames")]:
        for sets in ([t1, t1], [t0, t1]):
            with pytest.raises(D.DcsError) as e:
                gpu_ctx.encode93a_sweep(pcm, sets)
            assert e.value.status == status and word in str(e.value)
    with pytest.raises(D.DcsError) as e:                     # 65 535 frames cannot be measured: the extra frame would be the 65 536th
        gpu_ctx.encode93a_sweep([ok, np.zeros(65535 * 240, np.float32)], [t1])
    assert e.value.status == -1 and "stream 1" in str(e.value) and "65 535" in str(e.value)
    with pytest.raises(D.DcsError) as e:                     # the OS93 sweep keeps its refusal
        gpu_ctx.encode_sweep([ok], [D.encode93_params(D.OS93A), t1])
    assert e.value.status == -1 and "OS93a Type 1" in str(e.value)


def test_fit_chooses_between_the_layouts(gpu_ctx):
    q = A.DEFAULTS["maximumQuantizationError"]
    rates = [128000, 64000, None, 8000]                     # None: Type 0 at the defaults
    sets = [D.encode93a_params(D.FMT_93_T0) if r is None else D.encode93a_params(D.FMT_93A_T1, targetBitRate=r) for r in rates]
    restated = {}
    for name in C.NAMES:
        t0 = A.E93.encode(C.analysis(name)["x"], 0x9301, 0, **A.DEFAULTS)
        if t0[2] > 0:                                       # (a Type-0 stream that keeps no band cannot be measured)
            restated[name] = [t0[0] if r is None else A.encode_type1(C.analysis(name), targetBitRate=r)[0] for r in rates]
    names = list(restated)
    assert len(names) >= 6
    flat = [s for name in names for s in restated[name]]
    dec, err, first = gpu_ctx.decode_streams([(D.OS93A, s, 255, 0xFF) for s in flat], extra_frames=1)
    assert not err.any()
    n_bytes = [[len(s) for s in restated[name]] for name in names]
    sq_err = [[S.sq_err(S.measure(C.SIGNALS[name], dec[first[4 * i + r]:first[4 * i + r + 1]])) for r in range(4)] for i, name in enumerate(names)]
    col = [sum(row[r] for row in n_bytes) for r in range(4)]
    pcm = [C.SIGNALS[name] for name in names]
    moved = 0
    for budget in (col[0], (col[0] + col[1]) // 2):
        status, choice, total = S.fit(n_bytes, sq_err, budget)
        assert status == 0
        streams, got_choice, res, got_total = gpu_ctx.encode93a_fit(pcm, sets, budget)
        assert got_choice.tolist() == choice and got_total == total <= budget
        assert streams == [restated[name][choice[i]] for i, name in enumerate(names)]
        assert D.sweep_sq_err(res) == [sq_err[i][c] for i, c in enumerate(choice)]
        moved += len(set(choice)) > 1
    assert S.fit(n_bytes, sq_err, col[0])[1] == [0] * len(names) and moved == 1
    with pytest.raises(D.DcsError) as e:
        gpu_ctx.encode93a_fit(pcm, sets, min(col) - 1)
    assert e.value.status == -5 and e.value.needed == min(col)
