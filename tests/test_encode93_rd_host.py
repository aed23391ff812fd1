"""The rate-distortion OS93 Type-0 encoder without a GPU: what the numpy restatement (tests/enc93rd_ref.py) is made of -- the
tables, the quantiser, the frame trellis against exhaustive enumeration, the budget rules -- every stream of the grid through
the compiled reference decoder and the oracle to its last bit, what the cases reach, a few hashes that pin the restatement
(tests/golden/encode93_rd_golden.json), and the library's host-only side (exports, the bound, argument errors)."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

import enc93rd_cases as C
import enc93rd_ref as R

E = R.E
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "encode93_rd_golden.json")


def test_tables_and_constants(dcs):
    assert len(R.LADDER) == R.KL and R.LADDER[:6] == [0, 1, 2, 3, 4, 6] and R.LADDER[-1] == 1 << 32
    # M0 of OS93b is what dcs_stream_params gives at volume, level and channel volume 0xFF behind a fresh decoder's first
    # frame; OS93a's is DESIGN.md 10.10's (the library's value behind the volume scaling is 0xFFFA: 10.12, "Level")
    assert int(dcs.stream_params(dcs.OS93B, 0xFF, 0xFF, 3)[0][1]) == R.M0[C.B] == 0xFEFC and R.M0[C.A] == 0xFFFE
    # codes that share an integer scale: 0..3 are all 1
    assert E.SCALE[:4].tolist() == [1, 1, 1, 1] and R.QMAX[0] == 32767 and R.QMAX[63] == 32767 // int(E.SCALE[63])
    # the bounds DESIGN.md 10.12 states: a band's D, a frame's cost, the packed tie key, the sums over a stream
    band_d = 16 * 65535 ** 2
    assert band_d < 1 << 37 and R.E_MAX == 1 << 40
    frame_cost = 16 * (R.E_MAX + R.LADDER[-1] * 263)
    assert R.MAX_FRAME_BITS == 16 * 263 < 1 << 13 and frame_cost < 1 << 46 and (frame_cost << 13) < 1 << 62
    assert 16 * 65535 * (R.E_MAX + R.LADDER[-1] * 261) < R.INF < 1 << 63     # sixteen bands' proxy sums
    assert 65535 * 16 * band_d < 1 << 57 and 65535 * R.MAX_FRAME_BITS < 1 << 29          # a job's D and bits
    assert [int(v) for v in R.swidth(np.array([0, -1, 1, -2, 2, 127, 128, -128, -129, 32767, -32768, 32768, 65535, -65535]))] \
        == [1, 1, 2, 2, 3, 8, 9, 8, 9, 16, 16, 17, 17, 17]
    assert R.band_floor(0.0) == 0 and R.band_floor(1e6) == R.E_MAX and R.band_floor(2.0) == (1 << 32) * 16


@pytest.mark.parametrize("version", [C.A, C.B])
def test_the_quantiser_is_nearest(version):
    """for every scale code and every target, the four candidates contain a nearest value of all |q| <= QMAX[e]"""
    t = np.arange(-32768, 32768, dtype=np.int64)[:65535]
    got = R.nearest(t, version)                                     # [65535, 64]
    for e in range(64):
        q = np.arange(-R.QMAX[e], R.QMAX[e] + 1)
        r = R.recon(q, e, version)
        assert (np.diff(r) >= 0).all()                              # no wrap inside QMAX: the word is monotone in q
        pos = np.clip(np.searchsorted(r, t), 1, len(r) - 1)
        best = np.minimum(np.abs(t - r[pos - 1]), np.abs(t - r[pos]))
        assert np.array_equal(np.abs(t - R.recon(got[:, e], e, version)), best), e
        assert (np.abs(got[:, e]) <= R.QMAX[e]).all()
    assert np.abs(R.nearest(np.array([32767]), version)).max() <= R.QMAX.max()


def _enumerate(it, f, hv, n, lam, Eb):
    """every state sequence of frame f's first n bands in plain Python -> the least (cost, bits, sequence)"""
    fr = np.array([f])
    best = None
    for seq in itertools.product(range(R.NS), repeat=n):
        cost = bits = 0
        p, P, Dl = R.DDELTA, 0, 0
        for b, s in enumerate(seq):
            e = np.array([hv[b]])
            pP, pDl = np.zeros((1, R.NS), np.int64), np.zeros((1, R.NS), np.int64)
            pP[0, p], pDl[0, p] = P, Dl
            sb = int(_STEP(it, b, fr, e, pP, pDl, b == 0)[0, p, s])
            if sb < 0:
                cost = None
                break
            Ds, oP, oDl = _STATES(it, b, fr, e)
            cost += max(int(Ds[0, s]), Eb) + lam * sb
            bits += sb
            p, P, Dl = s, int(oP[0, s]), int(oDl[0, s])
        if cost is not None and (best is None or (cost, bits) < best[:2]):
            best = (cost, bits, seq)
    return best


_CACHE = {}


def _STEP(it, b, fr, e, pP, pDl, first):
    return R.step_bits(it, b, fr, e, pP, pDl, first)


def _STATES(it, b, fr, e):
    key = (id(it), b, int(fr[0]), int(e[0]))
    if key not in _CACHE:
        _CACHE[key] = R.band_states(it, b, fr, e)
    return _CACHE[key]


@pytest.mark.parametrize("name,frame", [("one_frame", 0), ("impulse_edge", 1)])
def test_the_frame_trellis_is_optimal_exhaustively(name, frame):
    """a fixed header, the first two bands, four ladder entries: every state sequence enumerated (19^2 of them, the steps
    that do not exist among them); the trellis's cost and bits are the least"""
    it = C.analysis(name, C.B)["it"]
    Eb = R.band_floor(C.MQE)
    for hv in ([20, 22], [30, 27]):
        for li in (0, 9, 20, 40):
            lam = R.LADDER[li]
            want = _enumerate(it, frame, hv, 2, lam, Eb)
            d, bits, st = R.trellis(it, np.array([frame]), np.array([hv + [0] * 14]), np.array([2]), np.array([lam], np.int64), Eb, True)
            Ds = [R.band_states(it, b, np.array([frame]), np.array([hv[b]]))[0][0, st[0, b]] for b in range(2)]
            assert int(d[0]) == sum(int(v) for v in Ds)
            assert sum(max(int(v), Eb) for v in Ds) + lam * int(bits[0]) == want[0] and int(bits[0]) == want[1], (hv, li)


@pytest.mark.parametrize("name,version,rate,mqe", C.GRID, ids=C.IDS)
def test_decoders_read_the_stream_to_its_last_bit(reference, oracle, dcs, name, version, rate, mqe):
    s, ch, rec, st = C.expected(name, version, rate, mqe)
    t = C.analysis(name, version)["t"]
    F = C.FRAMES[name]
    os_ = R.OS_OF[version]
    assert len(s) == 18 + (ch["frameBits"] + 7) // 8 and (s[0] << 8 | s[1]) == F
    assert all(v < 0x40 for v in s[2:2 + ch["numBands"]]) and all(v == 0xFF for v in s[2 + ch["numBands"]:18])
    assert not rec[:, 255].any() and not t[:, 255].any()            # sample 255: no target, value 0
    for checker in (reference, oracle):
        out, offs, _, stops = checker.decompress(os_, s + bytes(8), R.M0[version], F + 1)     # (one more: where the last frame ended)
        assert not stops[:F].any()
        assert offs[F] - offs[0] == ch["frameBits"]
        fb = out[:F, :256].astype(np.int16).astype(np.int64)
        assert np.array_equal(fb, R.frame_buffer(rec))
        assert not out[:F, 256:].any()
        assert int(((R.frame_buffer(t) - fb) ** 2).sum()) == ch["sqErr"]
    # the transition bit counts: the trellis's frame bits are the index pass's frame offsets
    it = C.analysis(name, version)["it"]
    rows = np.arange(F)
    _, bits, st2 = R.trellis(it, rows, np.tile(ch["hv"], (F, 1)), np.full(F, ch["numBands"]), np.full(F, R.LADDER[ch["ladderIndex"]], np.int64),
                             R.band_floor(mqe), True)
    assert np.array_equal(st2[:, :ch["numBands"]], st)
    idx, si = dcs.index_stream(os_, s)
    assert si.nFrames == F and len(idx) == F
    assert np.array_equal(idx["bitOff"].astype(np.int64) - int(idx["bitOff"][0]), np.concatenate([[0], np.cumsum(bits)[:-1]]))
    assert np.array_equal(idx["bitOff"].astype(np.int64) - int(idx["bitOff"][0]), offs[:F] - offs[0])
    assert len(s) <= dcs.encode93_rd_bound(len(C.SIGNALS[name])) == R.bound(len(C.SIGNALS[name]))


@pytest.mark.parametrize("name", ["one_frame", "level_step", "music"])
def test_budget_at_its_edge_and_one_bit_short(name):
    """the rate whose budget is exactly the generous stream's bits writes that stream; the rate one bit/s below does not"""
    F = C.FRAMES[name]
    for version in (C.A, C.B):
        top = C.expected(name, version, 5000000, 0.0)
        b = top[1]["frameBits"]
        assert top[1]["fits"]
        edge = -(-b * 31250 // (F * 240))                           # the least rate whose budget holds b bits
        at, below = C.expected(name, version, edge, 0.0), C.expected(name, version, edge - 1, 0.0)
        assert at[1]["budgetBits"] >= b > below[1]["budgetBits"]
        if F * 240 <= 31250:                                        # the budget moves a bit at a time
            assert at[1]["budgetBits"] == b == below[1]["budgetBits"] + 1
        assert at[0] == top[0] and at[1]["fits"] and C.info_tuple(at[1])[2:5] == C.info_tuple(top[1])[2:5]
        assert below[0] != top[0] and (not below[1]["fits"] or below[1]["frameBits"] <= below[1]["budgetBits"])
        assert below[1]["sqErr"] >= top[1]["sqErr"]
        # the byte form: at the stream's own length, and one byte short of it
        same = C.expected(name, version, 1, 0.0, len(top[0]))
        short = C.expected(name, version, 1, 0.0, len(top[0]) - 1)
        assert same[0] == top[0] and same[1]["budgetBits"] == 8 * (len(top[0]) - 18)
        assert len(short[0]) <= len(top[0]) - 1 and short[1]["fits"]


def test_budget_rules():
    name, version, mqe = "music", C.B, C.MQE
    F = C.FRAMES[name]
    sr = R.search(C.analysis(name, version), mqe)
    errs = []
    for budget in (17, 18, 19, 40, 100, 300, 700, 1500, 4000, 20000):
        st, c, _, _ = C.expected(name, version, 1, mqe, budget)
        fitting = [int(sr["D"][li]) for li in range(R.KL) if sr["bits"][li] <= c["budgetBits"] and budget >= 18]
        if c["fits"]:
            assert len(st) <= budget and c["sqErr"] == min(fitting)
        else:
            assert not fitting and c["frameBits"] == int(sr["bits"].min())
        errs.append(c["sqErr"])
    assert all(a >= b for a, b in zip(errs, errs[1:])), errs
    none = C.expected(name, version, 1, mqe, 17)[1]
    assert not none["fits"] and none["budgetBits"] == 0
    # budgetBytes and targetBitRate agree where they name the same bits
    bits = 62500 * F * 240 // 31250
    assert bits % 8 == 0
    a = C.expected(name, version, 62500, mqe)
    b = C.expected(name, version, 777, mqe, 18 + bits // 8)
    assert a[0] == b[0] and C.info_tuple(a[1]) == C.info_tuple(b[1])
    # the two versions reconstruct at different levels: different bytes for the same PCM
    assert any(C.expected(n, C.A, 96000, C.MQE)[0] != C.expected(n, C.B, 96000, C.MQE)[0] for n in C.SIGNALS)


def test_cases_reach_what_they_are_for():
    """Reached by the grid, all with legal PCM (no hand-made targets were needed): every direct code 1..15; the zero option
    with the reuse bit and without; the hold of band 0 and its reuse; a sub-type change in both directions; the delta and the
    double-delta option; numBands < 16 and == 1; two streams nothing fits; both versions, both error floors, 1, 2, 3, 17 and
    33 frames."""
    direct = set()
    n = dict.fromkeys(["zero with the reuse bit", "zero without", "hold", "hold reused", "delta", "double delta", "sub-type up",
                       "sub-type down", "numBands < 16", "numBands == 1", "does not fit", "delta behind a nonzero P"], 0)
    for g in C.GRID:
        s, ch, rec, st = C.expected(*g)
        prev = np.hstack([np.full((st.shape[0], 1), R.DDELTA), st[:, :-1]])
        direct |= set(st[(st >= 1) & (st <= 15)].tolist())
        n["zero with the reuse bit"] += int(((st == 0) & (prev == 0)).sum())
        n["zero without"] += int(((st == 0) & (prev != 0)).sum())
        n["hold"] += int((st[:, 0] == R.Z2).sum())
        n["hold reused"] += int(((st == R.Z2) & (prev == R.Z2)).sum())
        n["delta"] += int((st == R.DELTA).sum())
        n["double delta"] += int((st == R.DDELTA).sum())
        n["delta behind a nonzero P"] += int(((st >= R.DELTA) & (st != R.Z2) & ~R.CODE0[prev]).sum())
        up = R.SUB[st] == (R.SUB[prev] + 1) % 3
        n["sub-type up"] += int(up.sum())
        n["sub-type down"] += int((~up & (R.SUB[st] != R.SUB[prev])).sum())
        n["numBands < 16"] += ch["numBands"] < 16
        n["numBands == 1"] += ch["numBands"] == 1
        n["does not fit"] += not ch["fits"]
        assert not (st[:, 1:] == R.Z2)[prev[:, 1:] != R.Z2].any()   # the hold: behind the start state or itself alone
    print("\nreached: direct %s, %s" % (sorted(direct), n))
    assert direct == set(range(1, 16)) and all(n.values()), (direct, n)
    assert n["does not fit"] >= 2
    assert {g[1] for g in C.GRID} == {C.A, C.B} and {g[3] for g in C.GRID} == {0.0, C.MQE}
    assert {C.FRAMES[g[0]] for g in C.GRID} >= {1, 2, 3, 17, 33}


def test_restatement_is_pinned():
    golden = json.load(open(GOLDEN))
    assert len(golden["streams"]) >= 16
    for g in golden["streams"]:
        s, ch, _, _ = C.expected(g["signal"], g["version"], g["rate"], g["mqe"])
        assert (len(s), "%016x" % C.fnv1a64(s)) == (g["bytes"], g["fnv1a64"]), g
        assert list(C.info_tuple(ch)) == g["info"], g


def test_abi_exports_and_the_bound(dcs):
    from dcsexplorer_amd.api import EXPORTS, _ptr
    L = dcs.load_library()
    assert L.dcs_abi_version() == 9 == dcs.api.ABI_VERSION
    assert "dcs_encode93_rd_streams" in EXPORTS and "dcs_encode93_rd_bound" in EXPORTS
    for n in [0, 1, 239, 240, 241, 481, 240 * 65535, 240 * 65535 + 1]:
        assert dcs.encode93_rd_bound(n) == R.bound(n)
    assert dcs.encode93_rd_bound(240) == 18 + 526
    # without a context the call is refused before anything is written (what it says of bad parameters needs a context to
    # hold the message: tests/test_gpu_encode93_rd.py::test_calling_rules)
    x = np.zeros(240, np.float32)
    offs = np.array([0, 240], np.uint64)
    out, out_offs = np.zeros(64, np.uint8), np.zeros(2, np.uint64)
    p = dcs.encode93_params(dcs.OS93B, dcs.FMT_93_T0)
    assert L.dcs_encode93_rd_streams(None, _ptr(x), _ptr(offs), 1, ctypes.byref(p), None, _ptr(out), 64, _ptr(out_offs), None, None) == -1
    assert not out.any() and not out_offs.any()
    with pytest.raises(ValueError):
        dcs.Context.encode93_rd_streams(None, [x], dcs.OS94)
