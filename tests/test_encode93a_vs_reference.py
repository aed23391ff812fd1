"""The OS93a Type-1 restatement (tests/enc93a_ref.py) on the seeded adversarial cases of tests/enc93a_fuzz_cases.py, without a
GPU: every stream it writes goes through the compiled reference decoder and the oracle to its last bit, and through the
reference decoder's sanitizer build; the budget holds at its edge and one bit short of it; the wildcard's Type-0 side is
the compiled reference encoder's bytes; a few hashes pin the restatement (tests/golden/encode93a_fuzz_golden.json), so that
it and the kernels cannot drift together; and the cases reach what they were made for.  The restatement is what
tests/test_gpu_encode93a_vs_reference.py holds the kernels to."""
import concurrent.futures
import json
import os

import numpy as np
import pytest

import dec_cases
import enc93a_fuzz_cases as Z
import enc93a_ref as A
import enc_cases as X

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "encode93a_fuzz_golden.json")
LARGE_Q = 17500.0                       # from here the unbounded E_b of the widest band passed 2^64


def variants(name):
    """the (rate, q) a case is encoded at: its set's, the top rate, and the two computed rates at the budget's edge"""
    c = Z.CASES[name]
    edge, below = Z.edge_rates(name)
    return [(c.rate, c.q), (Z.TOP_RATE, c.q), (edge, c.q), (below, c.q)]


@pytest.mark.parametrize("name", Z.NAMES)
def test_reference_decoder_reads_the_stream_to_its_last_bit(reference, oracle, dcs, name):
    t = Z.analysis(name)["t"]
    F = t.shape[0]
    for rate, q in variants(name):
        s, ch, rec = Z.type1(name, rate, q)
        assert len(s) == 3 + (ch["frameBits"] + 7) // 8 and (s[0] << 8 | s[1]) == F == Z.FRAMES[name]
        assert s[2] == 0x80 | ch["selector"] << 5 | ch["numBands"] and 1 <= ch["numBands"] <= 18
        assert ch["budgetBits"] == rate * F * 240 // 31250
        for checker in (reference, oracle):
            out, offs, _, stops = checker.decompress(Z.OS93A, s, A.M0, F + 1)   # (one more: where the last frame ended)
            assert not stops[:F].any()
            assert offs[F] - offs[0] == ch["frameBits"]
            fb = out[:F, :254].astype(np.int16).astype(np.int64)
            assert np.array_equal(fb, rec)
            assert not out[:F, 254:].any()
            assert int(((t - fb) ** 2).sum()) == ch["sqErr"]
        idx, si = dcs.index_stream(Z.OS93A, s)
        assert si.nFrames == F and len(idx) == F
        assert np.array_equal(idx["bitOff"].astype(np.int64) - int(idx["bitOff"][0]), offs[:F] - offs[0])
        assert len(s) <= dcs.encode93a_bound(len(Z.CASES[name].pcm))


@pytest.mark.parametrize("name", Z.NAMES)
def test_budget_and_its_edge(name):
    c = Z.CASES[name]
    cands = Z.candidates(Z.walk(name, c.q))
    for rate, q in variants(name):
        ch = Z.type1(name, rate, q)[1]
        if ch["fits"]:
            assert ch["frameBits"] <= ch["budgetBits"]
            assert ch["sqErr"] == min(x[0] for x in cands if x[1] <= ch["budgetBits"])
        else:
            assert ch["frameBits"] == min(x[1] for x in cands) > ch["budgetBits"]
    top, edge, below = (Z.type1(name, rate, q)[1] for rate, q in variants(name)[1:])
    keys = ("selector", "ladderIndex", "numBands", "frameBits", "sqErr")
    assert top["fits"] and edge["fits"] and [edge[k] for k in keys] == [top[k] for k in keys]
    assert edge["budgetBits"] >= edge["frameBits"] > below["budgetBits"]
    if Z.FRAMES[name] * 240 <= 31250:                       # the budget moves a bit at a time: exactly at it, and one bit short
        assert edge["budgetBits"] == edge["frameBits"] == below["budgetBits"] + 1
    assert not below["fits"] or [below[k] for k in keys] != [top[k] for k in keys]
    assert Z.type1(name, *variants(name)[2])[0] == Z.type1(name, *variants(name)[1])[0]


def test_sanitizer_build_of_the_decoder_reports_value_shifts_only():
    """on every encoder-made stream: no masked-shift report (scale codes stay in 4..0x39), nothing that sets a case aside"""
    if not dec_cases.checker_available():
        pytest.skip("oracle/_ref/dcs_decref not built (needs the reference tree; `make -C oracle decref`)")
    cases = [Z.dec_case("%s@%d" % (name, rate), Z.type1(name, rate, q)[0]) for name in Z.NAMES for rate, q in variants(name)[:2]]
    refs = dec_cases.run_reference(cases, san=True)
    plain = dec_cases.run_reference(cases)
    shifts = 0
    for c, r, p in zip(cases, refs, plain):
        aside, value, masked = dec_cases.reports(r)
        assert r.kind == "decoded" and r.status == 0 and aside == [] and masked == 0, (c.name, aside, masked)
        assert np.array_equal(r.pcm, p.pcm), c.name
        shifts += value
    assert shifts > 0                                       # (the build does report: `<<` on negative values, on any stream)


@pytest.fixture(scope="module")
def type0_side():
    """enc_cases.check of every case as layout 93a/T0 at its set's params -> {name: Result}"""
    if not X.reference_available():
        pytest.skip(X.MISSING)
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        res = dict(zip(Z.NAMES, pool.map(lambda n: X.check(Z.enc_case(n)), Z.NAMES)))
    kept = sum(r.status == "kept" for r in res.values())
    print("\nType-0 side vs the reference encoder: kept %d of %d, dropped %s" % (kept, len(res), sorted(n for n, r in res.items() if r.status != "kept")))
    return res


def test_wildcard_type0_side_is_the_reference_encoders(type0_side):
    kept = [n for n, r in type0_side.items() if r.status == "kept"]
    assert len(kept) >= 0.9 * len(Z.NAMES), (len(kept), len(Z.NAMES))
    for name in kept:
        r = type0_side[name]
        assert r.ref == r.want == Z.type0(name)[0], name


@pytest.mark.parametrize("name", Z.NAMES)
def test_wildcard_is_the_first_strictly_smallest(name):
    c = Z.CASES[name]
    got = Z.expected(name, -1)
    one, zero = Z.type1(name)[0], Z.type0(name)[0]
    assert len(got[0]) == min(len(one), len(zero))
    assert (got[0], got[1]) == ((zero, 0) if len(zero) <= len(one) else (one, 1))
    s, typ, keep, ch = A.encode(Z.analysis(name), -1, **Z.params(c.rate, c.q))       # (the restatement's own wording of the rule)
    assert (s, typ, keep) == got[:3] and ch == got[3]


def test_both_types_win_somewhere():
    wins = [Z.expected(name, -1)[1] for name in Z.NAMES]
    assert 0 in wins and 1 in wins


def test_the_floor_saturates_and_nothing_changes_where_it_was_defined():
    """E_b is min(floor(...), 2^40).  Every D is below 2^38 (56 words x 65 535^2), so from E_b = 2^38 on max(D, E_b) = E_b for
    every option of the band and the walk picks its fewest bits: 2^38, 2^40 and the unbounded 2^200 choose alike."""
    assert 2 * int(A.INPUTS.max()) * 65535 ** 2 < 1 << 38
    for q in (17000.0, LARGE_Q, 18000.0, Z.Q_NEAR_2_64, 1e6, 1e30, float(np.finfo(np.float32).max)):
        assert [int(e) for e in A.band_floor(q)] == [1 << 40] * 18, q
    assert [int(e) for e in A.band_floor(-2.0)] == [int(e) for e in A.band_floor(2.0)] == [(1 << 32) * 2 * int(n) for n in A.INPUTS]
    assert [int(e) for e in A.band_floor(8.0)] == [min(1 << 40, (1 << 36) * 2 * int(n)) for n in A.INPUTS]      # both sides of it
    name = "full_scale/square_half1"
    D0, S0, D = (v.tolist() for v in Z.analysis(name)["search"])
    assert max(max(D0[1]), max(max(max(k) for k in w) for w in D[1])) < 1 << 38
    for c in range(4 * A.KL):
        got = [Z.walk_int(D0[1], S0[1], D[1], c // A.KL, A.LADDER[c % A.KL], [e] * 18) for e in (1 << 38, 1 << 40, 1 << 200)]
        assert all({k: g[k] for k in ("w", "s", "L", "through", "sumD")} == {k: got[0][k] for k in ("w", "s", "L", "through", "sumD")} for g in got), c
    # and the numpy walk under a saturated floor is that walk
    wk = A.walk(*Z.analysis(name)["search"], 18000.0)
    for c in (0, 70, 200, 255):
        o = Z.walk_int(D0[1], S0[1], D[1], c // A.KL, A.LADDER[c % A.KL], [1 << 200] * 18)
        assert o["w"] == wk["w"][1, c].tolist() and o["sumD"] == int(wk["sumD"][1, c]) and o["through"] == int(wk["through"][1, c])


def test_large_q_cases_are_there():
    large = [n for n in Z.NAMES if abs(Z.CASES[n].q) >= LARGE_Q]
    assert len(large) >= 15 and any(Z.analysis(n)["t"].any() for n in large)
    for n in large:                                         # every band floored: the fewest bits there are, a terminator a frame
        ch = Z.type1(n)[1]
        assert ch["frameBits"] == 4 * Z.FRAMES[n] and ch["numBands"] == 1 and ch["sqErr"] == int((Z.analysis(n)["t"] ** 2).sum())


def test_cases_reach_what_they_are_for():
    reached = dict.fromkeys(["cost tie broken by bits", "cost and bits tie broken by w or s", "sumD tie between candidates",
                             "two points tie for a pair", "unreachable delta", "no terminator anywhere",
                             "numBands == 1 with a coded band", "does not fit"] + ["selector %d" % pp for pp in range(4)], 0)
    lowest = A.PRV0
    for name in Z.NAMES:
        for rate, q in variants(name):
            f = Z.facts(name, rate, q)
            reached["cost tie broken by bits"] += f["bit_ties"] > 0
            reached["cost and bits tie broken by w or s"] += f["full_ties"] > 0
            reached["sumD tie between candidates"] += f["sumd_ties"] > 0
            reached["two points tie for a pair"] += f["point_ties"] > 0
            reached["unreachable delta"] += f["unreachable"] > 0
            reached["no terminator anywhere"] += f["no_terminator"] and Z.FRAMES[name] > 1
            reached["numBands == 1 with a coded band"] += f["one_band_coded"]
            reached["does not fit"] += not f["fits"]
            reached["selector %d" % f["selector"]] += 1
            lowest = min(lowest, f["prv"])
    print("\nreached (streams of %d): %s; lowest prv %d" % (4 * len(Z.NAMES), reached, lowest))
    assert all(reached.values()), reached
    assert lowest < 4 and Z.LOW_PRV_MIN < 4                 # (below 4 some scale codes have no delta)
    kinds = {c.kind for c in Z.CASES.values()}
    assert kinds >= {"quiet", "one_band", "gaps", "ramp", "low_prv", "full_scale", "long"} | {k for k, _ in X.KINDS if k != "silence"}
    assert {abs(c.q) for c in Z.CASES.values()} >= {abs(q) for q in Z.QS} and len({c.q for c in Z.CASES.values()}) >= 30
    assert Z.FULL_SCALE_PEAK == 30959                       # no legal input found that reaches the targets' clamp


def test_restatement_is_pinned():
    golden = json.load(open(GOLDEN))
    assert len(golden["streams"]) >= 16
    assert {g["signal"].split("/")[0] for g in golden["streams"]} >= {"quiet", "one_band", "gaps", "ramp", "low_prv", "full_scale", "long"}
    assert sum(abs(g["mqe"]) >= LARGE_Q for g in golden["streams"]) >= 3
    for g in golden["streams"]:
        s, ch, _ = Z.type1(g["signal"], g["rate"], g["mqe"])
        assert (len(s), "%016x" % Z.fnv1a64(s)) == (g["bytes"], g["fnv1a64"]), g
        assert [ch[k] for k in ("selector", "ladderIndex", "numBands", "frameBits", "sqErr")] == g["info"], g
