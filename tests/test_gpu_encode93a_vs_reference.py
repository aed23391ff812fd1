"""dcs_encode93a_streams, dcs_encode93a_sweep and Context.encode93a_fit on the MI355X over the seeded adversarial cases of
tests/enc93a_fuzz_cases.py: quiet signals whose costs, sums and points tie, the budget's edge and one bit short of it,
maximumQuantizationError up to float32's largest, streams without a terminator, silent frames between loud ones, 256 and 257
frames, more distinct q than two launches of A1 walk, random job lists under random group caps.  Expected bytes and records
come from the numpy restatement (tests/enc93a_ref.py, held to the compiled reference decoder and encoder by
tests/test_encode93a_vs_reference.py), the measured sums from tests/sweep_ref.py over the library's existing decoder's PCM
of the RESTATED bytes; nothing expected comes from the call under test."""
import numpy as np
import pytest

import dcsexplorer_amd as D
import enc93a_fuzz_cases as Z
import enc93a_ref as A
import sweep_ref as S

pytestmark = pytest.mark.gpu

FMT = {1: D.FMT_93A_T1, -1: None}
SUMS = ("nCompared", "sumSrcSq", "sumDecSq", "sumCross", "peakErr")


def _pcm(names):
    return [Z.CASES[n].pcm for n in names]


def _check(name, got, inf, infa, want):
    s, typ, keep, ch = want
    assert got == s, name
    assert (inf["formatType"], inf["formatSubType"], inf["nBytes"], inf["bandsToKeep"]) == (typ, 0, len(s), keep), name
    assert inf["nFrames"] == (s[0] << 8 | s[1]), name
    assert [int(infa[k]) for k in Z.INFO_KEYS] == [ch[k] for k in Z.INFO_KEYS], name


def _same(a, b):
    return a.shape == b.shape and bool((a == b).all())


@pytest.mark.parametrize("k", range(Z.N_SETS), ids=["set%d-%d-q%g" % (k, Z.rate_of(k), Z.QS[k]) for k in range(Z.N_SETS)])
def test_every_case_equals_the_restatement(gpu_ctx, k):
    names, rate, q = Z.SETS[k], Z.rate_of(k), Z.QS[k]
    for typ in (1, -1):
        streams, info, infa = gpu_ctx.encode93a_streams(_pcm(names), FMT[typ], **Z.params(rate, q))
        for j, name in enumerate(names):
            _check(name, streams[j], info[j], infa[j], Z.expected(name, typ))


def test_a_floor_beside_2_to_the_64(gpu_ctx):
    """q = 25 705.33: the unbounded E_b of the 13-pair band 17 is 2^36.7 short of 2^64 (and the 14-pair band's is past it),
    so without the saturation eb + lambda * bits wraps for the ladder's upper entries and a coded band 17 costs next to
    nothing; with it every band is absent"""
    names = ["s33/0/unit/479", "s26/0/impulse/481", "s25/1/music/481", "full_scale/dc", "one_band/04", "gaps/every17"]
    for rate in (Z.TOP_RATE, 64000):
        streams, info, infa = gpu_ctx.encode93a_streams(_pcm(names), D.FMT_93A_T1, **Z.params(rate, Z.Q_NEAR_2_64))
        for j, name in enumerate(names):
            want = Z.expected(name, 1, rate, Z.Q_NEAR_2_64)
            assert want[3]["frameBits"] == 4 * Z.FRAMES[name]
            _check(name, streams[j], info[j], infa[j], want)


@pytest.mark.parametrize("k", range(Z.N_SETS))
def test_batch_invariance(gpu_ctx, k):
    names, rate, q = Z.SETS[k], Z.rate_of(k), Z.QS[k]
    rng = np.random.default_rng([Z.SEED, 0xBA, k])
    order = [names[j] for j in rng.permutation(len(names))]
    for typ in (1, -1):
        streams, info, infa = gpu_ctx.encode93a_streams(_pcm(order), FMT[typ], **Z.params(rate, q))
        for j, name in enumerate(order):
            _check(name, streams[j], info[j], infa[j], Z.expected(name, typ))
    for name in [names[j] for j in rng.permutation(len(names))[:3]]:
        typ = int(rng.choice([1, -1]))
        streams, info, infa = gpu_ctx.encode93a_streams(_pcm([name]), FMT[typ], **Z.params(rate, q))
        _check(name, streams[0], info[0], infa[0], Z.expected(name, typ))


def test_the_budgets_edge_and_one_bit_short(gpu_ctx):
    """every case at its two computed rates, a job each: one sweep call with per-stream parameters"""
    sets, jobs, want = [], [], []
    for i, name in enumerate(Z.NAMES):
        for rate in Z.edge_rates(name):
            jobs.append((i, len(sets)))
            sets.append(D.encode93a_params(D.FMT_93A_T1, **Z.params(rate, Z.CASES[name].q)))
            want.append((name, rate))
    streams, res, infa = gpu_ctx.encode93a_sweep(_pcm(Z.NAMES), sets, jobs, measure=False)
    exact = 0
    for j, (name, rate) in enumerate(want):
        s, ch, _ = Z.type1(name, rate)
        assert streams[j] == s, (name, rate)
        assert [int(infa[j][k]) for k in Z.INFO_KEYS] == [ch[k] for k in Z.INFO_KEYS], (name, rate)
        assert (res["enc"][j]["formatType"], res["enc"][j]["nBytes"], res["enc"][j]["bandsToKeep"]) == (1, len(s), ch["numBands"])
        exact += ch["frameBits"] == ch["budgetBits"]
    assert exact >= len(Z.NAMES) - 3                         # (all but the streams of more than 130 frames)


# the sweep: 20 distinct q (three launches of A1), a Type-0 set among them, and a few cases' computed edge rates
SWEEP_KS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 14, 16, 19, 21, 27, 30, 31, 33, 34]
EDGE_NAMES = [n for n in Z.NAMES if Z.CASES[n].set in (0, 5, 12, 16) and Z.FRAMES[n] <= 17][:6]
T0_AT = 3


def _sweep_sets():
    """[(rate, q) or None for the Type-0 set]"""
    out = [(Z.rate_of(k), Z.QS[k]) for k in SWEEP_KS]
    for n in EDGE_NAMES:
        out += [(r, Z.CASES[n].q) for r in Z.edge_rates(n)]
    out.insert(T0_AT, None)
    return out


def _sweep_jobs(sets):
    """a seeded random job list with repeats: short streams under any set, each edge rate with its own stream, the long
    streams under their own q"""
    rng = np.random.default_rng([Z.SEED, 0x5E])
    short = [i for i, n in enumerate(Z.NAMES) if Z.FRAMES[n] <= 17]
    jobs = [(int(rng.choice(short)), int(rng.integers(len(sets)))) for _ in range(90)]
    at = len(SWEEP_KS) + 1
    for j, n in enumerate(EDGE_NAMES):
        jobs += [(Z.NAMES.index(n), at + 2 * j), (Z.NAMES.index(n), at + 2 * j + 1)]
    for n in Z.NAMES:
        if Z.FRAMES[n] > 17 and Z.CASES[n].set in SWEEP_KS:
            r = SWEEP_KS.index(Z.CASES[n].set)
            jobs.append((Z.NAMES.index(n), r + (r >= T0_AT)))
    jobs = [jobs[j] for j in rng.permutation(len(jobs))]
    return jobs + [jobs[5], jobs[5], jobs[17]]


@pytest.fixture(scope="module")
def swept(gpu_ctx):
    sets = _sweep_sets()
    assert len({q for rq in sets if rq for q in [rq[1]]}) == 20 and sets[T0_AT] is None
    params = [D.encode93a_params(D.FMT_93_T0) if rq is None else D.encode93a_params(D.FMT_93A_T1, **Z.params(*rq)) for rq in sets]
    jobs = _sweep_jobs(sets)
    assert len(set(jobs)) < len(jobs) and any(sets[r] is None for _, r in jobs)
    assert any(Z.FRAMES[Z.NAMES[i]] >= 256 for i, _ in jobs)
    return sets, params, jobs, gpu_ctx.encode93a_sweep(_pcm(Z.NAMES), params, jobs)


def test_sweep_jobs_equal_the_restatement(swept):
    sets, params, jobs, (streams, res, infa) = swept
    assert len(streams) == len(jobs) == len(res) == len(infa)
    for j, (i, r) in enumerate(jobs):
        name, e = Z.NAMES[i], res["enc"][j]
        if sets[r] is None:
            t0 = Z.type0(name, A.DEFAULTS["targetBitRate"], A.DEFAULTS["maximumQuantizationError"])
            assert streams[j] == t0[0] and (e["formatType"], e["nBytes"], e["bandsToKeep"]) == (0, len(t0[0]), t0[2]), (name, r)
            assert not any(int(infa[j][k]) for k in Z.INFO_KEYS), (name, r)
            continue
        s, ch, _ = Z.type1(name, *sets[r])
        assert streams[j] == s, (name, r)
        assert (e["formatType"], e["formatSubType"], e["nFrames"], e["nBytes"], e["bandsToKeep"]) == (1, 0, Z.FRAMES[name], len(s), ch["numBands"])
        assert [int(infa[j][k]) for k in Z.INFO_KEYS] == [ch[k] for k in Z.INFO_KEYS], (name, r)


def test_sweep_sums_are_the_restated_streams(gpu_ctx, swept):
    sets, params, jobs, (streams, res, infa) = swept
    t1 = sorted({(i, r) for i, r in jobs if sets[r] is not None})
    pcm, err, first = gpu_ctx.decode_streams([(D.OS93A, Z.type1(Z.NAMES[i], *sets[r])[0], 255, 0xFF) for i, r in t1], extra_frames=1)
    assert not err.any()
    want = {ir: S.measure(Z.CASES[Z.NAMES[ir[0]]].pcm, pcm[first[k]:first[k + 1]]) for k, ir in enumerate(t1)}
    for j, ir in enumerate(jobs):
        if sets[ir[1]] is not None:
            assert res[j]["measured"] == 1 and {k: int(res[j][k]) for k in SUMS} == want[ir], (Z.NAMES[ir[0]], ir[1])
    assert any(int(r["peakErr"]) > 0 for r in res)


def test_sweep_under_group_caps(gpu_ctx, swept):
    sets, params, jobs, (streams, res, infa) = swept
    longest = max(Z.FRAMES[Z.NAMES[i]] for i, _ in jobs)
    try:
        for cap in (1, 7, longest):
            D.encode_sweep_group_frames(cap)
            got, res_g, infa_g = gpu_ctx.encode93a_sweep(_pcm(Z.NAMES), params, jobs)
            assert got == streams and _same(res_g, res) and _same(infa_g, infa), cap
    finally:
        D.encode_sweep_group_frames(0)


FIT_RATES = [128000, 48000, 16000, 4000]


def test_fit_against_the_restatement(gpu_ctx):
    names = [n for n in Z.NAMES if 2 <= Z.FRAMES[n] <= 17 and Z.analysis(n)["t"].any()][:14]
    assert len(names) == 14
    q = A.DEFAULTS["maximumQuantizationError"]
    sets = [D.encode93a_params(D.FMT_93A_T1, **Z.params(r, q)) for r in FIT_RATES]
    restated = [[Z.type1(n, r, q)[0] for r in FIT_RATES] for n in names]
    k = len(FIT_RATES)
    dec, err, first = gpu_ctx.decode_streams([(D.OS93A, s, 255, 0xFF) for row in restated for s in row], extra_frames=1)
    assert not err.any()
    n_bytes = [[len(s) for s in row] for row in restated]
    sq_err = [[S.sq_err(S.measure(Z.CASES[n].pcm, dec[first[k * i + r]:first[k * i + r + 1]])) for r in range(k)] for i, n in enumerate(names)]
    col = [sum(row[r] for row in n_bytes) for r in range(k)]
    lo, hi = min(col), max(col)
    assert lo < hi
    moved = mixed = 0
    for budget in (lo + (hi - lo) // 4, lo + (hi - lo) // 2, lo + 3 * (hi - lo) // 4):
        status, choice, total = S.fit(n_bytes, sq_err, budget)
        assert status == 0
        streams, got_choice, res, got_total = gpu_ctx.encode93a_fit(_pcm(names), sets, budget)
        assert got_choice.tolist() == choice and got_total == total <= budget
        assert streams == [restated[i][c] for i, c in enumerate(choice)]
        assert D.sweep_sq_err(res) == [sq_err[i][c] for i, c in enumerate(choice)]
        moved += any(c != 0 for c in choice)
        mixed += len(set(choice)) > 1
    assert moved >= 1 and mixed >= 1


def test_round_trip_of_every_case(gpu_ctx, reference):
    """every case at its set's parameters, a job each; what the GPU wrote decodes on the GPU to what the reference decodes"""
    sets = [D.encode93a_params(D.FMT_93A_T1, **Z.params(Z.rate_of(k), Z.QS[k])) for k in range(Z.N_SETS)]
    jobs = [(i, Z.CASES[n].set) for i, n in enumerate(Z.NAMES)]
    streams, res, infa = gpu_ctx.encode93a_sweep(_pcm(Z.NAMES), sets, jobs, measure=False)
    for j, n in enumerate(Z.NAMES):
        assert streams[j] == Z.type1(n)[0], n
    got, err, first = gpu_ctx.decode_streams([(D.OS93A, s, 255, 0xFF) for s in streams])
    assert not err.any()
    for j, (n, s) in enumerate(zip(Z.NAMES, streams)):
        want = reference.decode(D.OS93A, 255, [s], [0xFF], Z.FRAMES[n])
        assert np.array_equal(got[first[j]:first[j + 1]], want), n
