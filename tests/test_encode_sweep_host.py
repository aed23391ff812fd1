"""dcs_encode_fit against its restatement (tests/sweep_ref.py), and the restated measurement against what the compiled
reference encoder and decoder make of the golden recordings (tests/golden/sweep_golden.json).  No GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc_ref as E
import sweep_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "sweep_golden.json")))["cases"]
ARR = np.load(os.path.join(HERE, "golden", "encode_golden.npz"))


def _tables(rng):
    """random [n][k] tables: mostly falling sizes and rising errors, with non-monotone columns, equal errors and equal sizes"""
    n, k = int(rng.integers(1, 9)), int(rng.integers(1, 7))
    kind = rng.integers(0, 4)
    if kind == 0:               # small values: many ties
        nb = rng.integers(1, 6, (n, k))
        se = rng.integers(0, 4, (n, k))
    else:
        base = rng.integers(100, 100000, (n, 1))
        nb = (base * np.sort(rng.uniform(0.1, 1.0, (n, k)), axis=1)[:, ::-1]).astype(np.int64) + 18
        se = (rng.integers(1, 1 << 40, (n, 1)) * np.sort(rng.uniform(0.5, 8.0, (n, k)), axis=1)).astype(np.int64)
        if kind >= 2:           # neither size nor error is monotone per stream
            for _ in range(int(rng.integers(1, 4))):
                i, a, b = rng.integers(0, n), rng.integers(0, k), rng.integers(0, k)
                nb[i, a], nb[i, b] = nb[i, b], nb[i, a]
                i, a, b = rng.integers(0, n), rng.integers(0, k), rng.integers(0, k)
                se[i, a], se[i, b] = se[i, b], se[i, a]
        if kind == 3:
            se[rng.integers(0, n)] = se[rng.integers(0, n)]             # equal errors across two streams
            nb[:, rng.integers(0, k)] = nb[:, rng.integers(0, k)]       # two equal columns of sizes
    return nb.astype(np.uint64), se.astype(np.uint64)


def _budgets(rng, nb):
    col = [int(c) for c in nb.sum(axis=0)]
    out = [min(col) - 1, min(col), max(col), max(col) + 1, col[0], col[0] + 1, col[-1], 0, 1 << 62]
    out += [int(rng.integers(min(col), max(col) + 2)) for _ in range(3)]
    out += [(a + b) // 2 for a, b in zip(col, col[1:])]
    return [b for b in out if b >= 0]


def test_fit_equals_the_restatement_on_seeded_tables():
    rng = np.random.default_rng(0xF17)
    n_cases = n_capacity = n_moved = 0
    for _ in range(600):
        nb, se = _tables(rng)
        for budget in _budgets(rng, nb):
            status, choice, total = S.fit(nb.tolist(), se.tolist(), budget)
            if status == 0:
                got_choice, got_total = D.encode_fit_choose(nb, se, budget)
                assert got_total <= budget
                assert got_total == sum(int(nb[i, c]) for i, c in enumerate(got_choice))
                n_moved += len(set(got_choice.tolist())) > 1
            else:
                with pytest.raises(D.DcsError) as e:
                    D.encode_fit_choose(nb, se, budget)
                assert e.value.status == -5
                got_choice, got_total = e.value.choice, e.value.needed
                assert got_total == min(int(c) for c in nb.sum(axis=0)) > budget
                n_capacity += 1
            assert got_choice.tolist() == choice and got_total == total, (nb, se, budget)
            n_cases += 1
    assert n_cases > 3000 and n_capacity > 300 and n_moved > 300


def test_fit_by_hand():
    # column totals 30, 20, 12; budget 25 -> r = 1 (20 bytes).  Visits by error at r: stream 2 (60), 0 (50), 1 (40).  Stream 2
    # moves to set 0 for nothing (10 bytes either way); stream 0 would make it 27; stream 1's error at set 0 is not smaller.
    # Budget 19 -> r = 2 (12 bytes), all errors equal there, so by index: 0 -> set 1 (13), 1 -> set 0 (17), 2 finds no room.
    nb = [[12, 5, 4], [8, 5, 4], [10, 10, 4]]
    se = [[1, 50, 90], [70, 40, 90], [5, 60, 90]]
    for budget, want in [(25, ([1, 1, 0], 20)), (26, ([1, 1, 0], 20)), (27, ([0, 1, 0], 27)), (29, ([0, 1, 0], 27)),
                         (30, ([0, 0, 0], 30)), (12, ([2, 2, 2], 12)), (19, ([1, 0, 2], 17)), (20, ([1, 1, 0], 20))]:
        choice, total = D.encode_fit_choose(nb, se, budget)
        assert (choice.tolist(), total) == want, budget
        assert S.fit(nb, se, budget) == (0,) + want
    # the visit order decides who gets the room: with 7 spare bytes stream 0 (error 50 at r) goes before stream 1 (40)
    nb = [[12, 5], [12, 5]]
    se = [[1, 50], [1, 40]]
    assert D.encode_fit_choose(nb, se, 17)[0].tolist() == [0, 1] and S.fit(nb, se, 17) == (0, [0, 1], 17)
    with pytest.raises(D.DcsError) as e:
        D.encode_fit_choose(nb, se, 9)
    assert e.value.status == -5 and e.value.needed == 10 and e.value.choice.tolist() == [1, 1]


def test_fit_argument_errors():
    import ctypes
    from dcsexplorer_amd.api import _ptr
    L = D.load_library()
    nb, se, ch, tot = np.ones(4, np.uint64), np.ones(4, np.uint64), np.zeros(2, np.int32), ctypes.c_uint64(0)
    assert L.dcs_encode_fit(_ptr(nb), _ptr(se), 2, 2, 100, _ptr(ch), ctypes.byref(tot)) == 0
    for args in [(None, _ptr(se), 2, 2), (_ptr(nb), None, 2, 2), (_ptr(nb), _ptr(se), 0, 2), (_ptr(nb), _ptr(se), 2, 0)]:
        assert L.dcs_encode_fit(*args, 100, _ptr(ch), ctypes.byref(tot)) == -1
    assert L.dcs_encode_fit(_ptr(nb), _ptr(se), 2, 2, 100, None, ctypes.byref(tot)) == -1
    assert L.dcs_encode_fit(_ptr(nb), _ptr(se), 2, 2, 100, _ptr(ch), None) == -1
    with pytest.raises(ValueError):
        D.encode_fit_choose([[1, 2]], [[1, 2], [3, 4]], 5)


def test_result_record_layout():
    assert D.SWEEP_RESULT_DTYPE.itemsize == 64 and D.SWEEP_JOB_DTYPE.itemsize == 8
    assert [D.SWEEP_RESULT_DTYPE.fields[k][1] for k in ("enc", "measured", "peakErr", "nCompared", "sumSrcSq", "sumDecSq", "sumCross")] \
        == [0, 20, 24, 32, 40, 48, 56]
    assert D.sweep_sq_err(np.array([((0, 0, 1, 20, 3), 1, 2, 240, 10, 20, 7)], D.SWEEP_RESULT_DTYPE)) == [16]


def test_measure_by_hand():
    x = np.array([0.5, -1.0, 1.0, 1.5 / 32768, 2.5 / 32768, -0.25], np.float32)     # rint: ties to even; +1.0 clamps to 32767
    assert S.quantise(x).tolist() == [16384, -32768, 32767, 2, 2, -8192]
    dec = np.zeros((2, 240), np.int16)
    dec[0, 16:22] = [16384, -32768, 32767, 0, 5, -8000]
    m = S.measure(x, dec)
    assert m == dict(nCompared=6, sumSrcSq=sum(v * v for v in S.quantise(x).tolist()),
                     sumDecSq=16384 ** 2 + 32768 ** 2 + 32767 ** 2 + 25 + 8000 ** 2,
                     sumCross=16384 ** 2 + 32768 ** 2 + 32767 ** 2 + 10 + 8192 * 8000, peakErr=192)
    assert S.sq_err(m) == 4 + 9 + 192 ** 2
    assert S.quantise(np.array([-7, 32767, -32768], np.int16)).tolist() == [-7, 32767, -32768]


@pytest.mark.parametrize("signal", ["rec0", "rec1", "rec2", "rec3"])
def test_measure_matches_the_compiled_reference(oracle, signal):
    """the restated encoder's bytes are the reference encoder's, and the restated measurement of the oracle's decode is
    the one recorded from the reference decoder's"""
    x = ARR[signal + "/pcm"]
    cases = [c for c in GOLDEN if c["signal"] == signal]
    assert [c["targetBitRate"] for c in cases] == list(S.RATES)
    for c in cases:
        stream, win, _ = E.encode(x, (-1, -1), targetBitRate=c["targetBitRate"])
        assert len(stream) == c["bytes"] and hashlib.sha256(stream).hexdigest() == c["sha256"] and list(win) == c["winner"]
        dec = oracle.decode(D.OS95 if win[1] == 3 else D.OS94, 255, [stream], [255], c["nFrames"] + 1)
        m = S.measure(x, dec)
        assert m == {k: c[k] for k in m}, (signal, c["targetBitRate"])
        assert S.sq_err(m) == c["sqErrAtLag"][S.LAG]


def test_the_findings_the_feature_rests_on():
    # the decoder's overlap: lag 16 has the smallest squared error of lags 0..255, for every recording and rate
    for c in GOLDEN:
        assert int(np.argmin(c["sqErrAtLag"])) == S.LAG and c["sqErrAtLag"].count(min(c["sqErrAtLag"])) == 1
    # the batch totals fall strictly with the bit rate ...
    totals = [sum(c["bytes"] for c in GOLDEN if c["targetBitRate"] == r) for r in S.RATES]
    assert all(a > b for a, b in zip(totals, totals[1:])), totals
    # ... while a stream's error does not: rec0 is worse at 256 k than at 192 k
    err = {(c["signal"], c["targetBitRate"]): c["sqErrAtLag"][S.LAG] for c in GOLDEN}
    assert err[("rec0", 256000)] > err[("rec0", 192000)]
