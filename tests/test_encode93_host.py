"""The OS93 encoder's host side, without a GPU: the numpy restatement (tests/enc93_ref.py) against the reference encoder's
own OS93 streams (tests/golden/encode93_golden.*), the library's header derivation (dcs_encode93_header) against both, the
size bound, the refusals, the oracle decoding what enc93_ref writes, and the Keep +15 rule."""
import hashlib
import json
import os

import numpy as np
import pytest

import enc_ref as E
import enc93_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "encode93_golden.json")))
ARR = np.load(os.path.join(HERE, "golden", "encode93_golden.npz"))
PCM = np.load(os.path.join(HERE, "golden", "encode_golden.npz"))
CASES = GOLDEN["cases"]
SHORT = [c for c in CASES if c["signal"] != GOLDEN["long"]["signal"]]
FMTS = {(0x9302, -1), (0x9302, 0), (0x9302, 1), (0x9301, 0), (0x9301, -1)}


def same_as_golden(case, s):
    """the reference's stream: its length and sha256, and its bytes where the fixture keeps them"""
    key = case["name"] + "/stream"
    if key in ARR.files and s != ARR[key].tobytes():
        return False
    return len(s) == case["bytes"] and hashlib.sha256(s).hexdigest() == case["sha256"]


def pcm_of(case):
    return PCM[case["signal"] + "/pcm"]


def test_golden_covers_the_issue_cases():
    asked = {}
    for c in CASES:
        asked.setdefault(c["signal"], set()).add((c["version"], c["type"]))
    for sig in ["rec%d" % v for v in range(4)] + ["len1", "len239", "len240", "len241", "silence", "dc", "square", "noise_fs",
                                                   "sine40", "near_silent", "float_tones"]:
        assert asked[sig] == FMTS, sig
    rates = {c["params"]["targetBitRate"] for c in CASES}
    assert {8000, 16000, 32000, 64000, 128000, 256000} <= rates
    assert {0.0, float(np.float32(0.9)), 1.0} <= {c["params"]["powerBandCutoff"] for c in CASES}
    assert min(c["params"]["maximumQuantizationError"] for c in CASES) < 10 / 32768
    assert any(c["nFrames"] == 65535 for c in CASES)
    assert all(set(c["ubsan"]) <= {"shift"} for c in CASES) and not GOLDEN["dropped"]
    assert {c["winner"] for c in CASES if c["version"] == 0x9302 and c["type"] == -1} == {0, 1}   # both layouts win somewhere
    # no golden input reaches the Keep +15 rule (test_keep_plus_15_rule pins it)
    assert not any(c["rules"] for c in CASES)
    assert sum(c["name"] + "/stream" in ARR.files for c in CASES) >= 30


@pytest.mark.parametrize("case", SHORT, ids=[c["name"] for c in SHORT])
def test_enc93_ref_reproduces_the_reference_encoder(case):
    s, win, _, fired = R.encode(pcm_of(case), case["version"], case["type"], **case["params"])
    assert same_as_golden(case, s)
    assert win == case["winner"] and fired == 0


def test_os93a_type0_equals_os93b_type0():
    by = {}
    for c in CASES:
        by.setdefault((c["signal"], tuple(sorted(c["params"].items()))), {})[(c["version"], c["type"])] = c["sha256"]
    n = 0
    for k, v in by.items():
        if (0x9301, 0) in v and (0x9302, 0) in v:
            assert v[0x9301, 0] == v[0x9302, 0], k
            n += 1
        if (0x9301, -1) in v and (0x9301, 0) in v:
            assert v[0x9301, -1] == v[0x9301, 0], k          # the 0x9301 wildcard tries Type 0 only
    assert n >= 15
    x = pcm_of(SHORT[0])
    assert R.encode(x, 0x9301, 0)[0] == R.encode(x, 0x9302, 0)[0]


def _stats(case):
    _, st = R.analyse_stream(E.to_float(pcm_of(case)))
    return st


@pytest.mark.parametrize("case", SHORT[::3], ids=[c["name"] for c in SHORT[::3]])
def test_encode93_header_matches_golden_headers(dcs, case):
    ps, lo, hi = _stats(case)
    os_ = dcs.OS93A if case["version"] == 0x9301 else dcs.OS93B
    hdr, keep, bits = dcs.encode93_header(ps, lo, hi, case["winner"], os_, **case["params"])
    assert hdr.tobytes().hex() == case["header"]
    rh, rk, rb = R.header(ps, lo, hi, case["winner"], dict(R.DEFAULTS, **case["params"]))
    assert rh.tobytes().hex() == case["header"] and keep == rk and list(bits) == list(rb)


def test_encode93_header_matches_enc93_ref_on_random_statistics(dcs):
    rng = np.random.default_rng(0x93EAD)
    shifts = set()
    for k in range(300):
        scale = 10.0 ** rng.uniform(-8, 1)
        ps = (rng.exponential(1.0, 16) * scale * np.where(rng.random(16) < 0.2, 1e-6, 1.0)).astype(np.float32)
        if k % 7 == 0:
            ps[rng.integers(1, 16):] = 0
        lo = (-rng.exponential(0.3, 16)).astype(np.float32)
        hi = rng.exponential(0.3, 16).astype(np.float32)
        p = dict(powerBandCutoff=float(np.float32(rng.choice([0.0, 0.5, 0.9, 0.97, 0.999, 1.0]))),
                 targetBitRate=int(rng.choice([1000, 8000, 32000, 128000, 256000, 1000000])))
        for typ in (0, 1):
            hdr, keep, bits = dcs.encode93_header(ps, lo, hi, typ, dcs.OS93B, **p)
            rh, rk, rb = R.header(ps, lo, hi, typ, dict(R.DEFAULTS, **p))
            assert hdr.tobytes() == rh.tobytes() and keep == rk and list(bits) == list(rb), (k, typ)
            shifts.update(int(b) for b in bits[:keep])
        h0, _, _ = dcs.encode93_header(ps, lo, hi, 0, dcs.OS93A, **p)
        assert h0.tobytes() == dcs.encode93_header(ps, lo, hi, 0, dcs.OS93B, **p)[0].tobytes()
    assert max(shifts) >= 32


def test_encode93_bound(dcs):
    # Type 1: 16 bands of 1 + 30 bits of flag and code, 15-bit samples, 15 in band 0 -> 4 321 bits a frame (Type 0: 4 208)
    assert 16 * 31 + (15 + 15 * 16) * 15 == 4321 and 16 * (1 + 2 + 4 + 16 * 16) == 4208
    for n in (1, 240, 241, 24000, 65535 * 240):
        nf = (n + 239) // 240
        assert dcs.encode93_bound(n) == 18 + (nf * 4321 + 7) // 8 == R.bound(n)
    assert dcs.encode93_bound(0) == 0 and dcs.encode93_bound(65535 * 240 + 1) == 0
    for c in CASES:
        n = len(pcm_of(c)) if c in SHORT else c["nFrames"] * 240
        assert c["bytes"] <= dcs.encode93_bound(n)
    assert dcs.encode_bound(240) == 18 + (16 * 23 + 255 * 15 + 7) // 8     # the 1994+ bound is unchanged


def test_encoder93_functions_are_exported(dcs):
    from dcsexplorer_amd.api import EXPORTS
    L = dcs.load_library()
    for name in ("dcs_encode93_bound", "dcs_encode93_header", "dcs_encode93_streams"):
        assert name in EXPORTS and hasattr(L, name)


def test_encode93_refuses_bad_arguments(dcs):
    z = np.full(16, 0.01, np.float32)
    for typ, os_, kw in [(1, dcs.OS93A, {}), (2, dcs.OS93B, {}), (0, dcs.OS93B, dict(formatVersion=0x9400)),
                         (0, dcs.OS93B, dict(formatVersion=0x9303)), (0, dcs.OS93B, dict(streamFormatSubType=4)),
                         (0, dcs.OS93B, dict(streamFormatType=2)), (0, dcs.OS93A, dict(streamFormatType=1)),
                         (0, dcs.OS93B, dict(targetBitRate=0))]:
        with pytest.raises(dcs.DcsError) as e:
            dcs.encode93_header(z, -z, z, typ, os_, **kw)
        assert e.value.status == -1, (typ, os_, kw)
    for sub in (-1, 0, 1, 2, 3):                          # OS93 has no sub-types: any of -1..3 is accepted and ignored
        assert dcs.encode93_header(z, -z, z, 0, dcs.OS93B, streamFormatSubType=sub)[0].tobytes() == \
            dcs.encode93_header(z, -z, z, 0, dcs.OS93B)[0].tobytes()
    # the 1994+ entry points still refuse OS93 versions
    with pytest.raises(dcs.DcsError):
        dcs.encode_header(z, -z, z, 0, 0, formatVersion=0x9302)
    # layouts that do not exist for an OS are refused in Python
    for os_, fmt in [(dcs.OS93A, dcs.FMT_93B_T1), (dcs.OS93B, dcs.FMT_93A_T1), (dcs.OS94, None), (dcs.OS93B, dcs.FMT_94_T0)]:
        with pytest.raises(ValueError):
            dcs.encode93_params(os_, fmt)
    assert dcs.encode93_params(dcs.OS93A, dcs.FMT_93A_T1).streamFormatType == 1       # refused by the library, not here


@pytest.mark.parametrize("version,typ,os_", [(0x9301, 0, 0), (0x9302, 0, 1), (0x9302, 1, 1)])
def test_enc93_ref_streams_decode_through_the_oracle(oracle, version, typ, os_):
    """the decoder stays in step: every frame starts where the encoder's frame bits say, and the last ends in the last byte"""
    rng = np.random.default_rng(0xDEC93 + typ)
    sigs = [PCM["rec%d/pcm" % v] for v in range(4)] + [PCM["noise_fs/pcm"], PCM["silence/pcm"]]
    sigs.append((0.4 * rng.standard_normal(240 * 40)).clip(-1, 1).astype(np.float32))
    for x in sigs:
        for rate in (16000, 128000):
            p = dict(R.DEFAULTS, targetBitRate=rate)
            an = R.analyse_stream(E.to_float(x))
            s, keep, _ = R.encode_layout(an, typ, p)
            f = an[0]
            F = f.shape[0]
            hdr, keep, _ = R.header(*an[1], typ, p)
            recs = R.records(f, hdr, keep, typ, p)
            w, _ = R.walk(recs, keep, typ, F)
            _, lens = R.emit(recs, w, keep, typ, F)
            frame_bits = lens.reshape(F, -1).sum(axis=1) if keep else np.zeros(F, np.int64)
            pcm, pr = oracle.decode(os_, 255, [s], [0x64], F, probes=True)
            starts = [pr[j].bitOff for j in range(F)]
            assert starts == list(np.concatenate([[0], np.cumsum(frame_bits)[:-1]])), (version, typ, rate)
            assert (len(s) - 18) * 8 - 8 < int(frame_bits.sum()) <= (len(s) - 18) * 8 or len(s) == 18


def _rec(s, best, best15=None):
    s = np.array([s], np.int64)
    d1 = np.diff(s, axis=1)
    return dict(s=s, best=np.array([best]), best15=np.array([best if best15 is None else best15]),
                L1=R.bitlen(np.abs(d1).max(axis=1)), L2=R.bitlen(np.abs(np.diff(d1, axis=1)).max(axis=1)))


def test_keep_plus_15_rule():
    """A Type-1 band after a sub-type-1 band, whose sub-type-1 code is 15 over a carried code of 0: the reference writes
    Keep +15, which has no code (length 0), and the decoder falls out of step.  The library keeps the sub-type-0 code."""
    assert R.BT_LEN[0, 15 + 16] == 0 and R.BT_LEN[1, 15 + 16] > 0       # Keep has no +15, Invert has
    assert all(R.BT_LEN[0, d + 16] > 0 for d in range(-15, 15)) and all(R.BT_LEN[1, d + 16] > 0 for d in range(-16, 16))
    recs = [_rec([0] * 15, 3),                    # all equal to prvSample 0: sub-type 1, code 0 (Invert)
            _rec([8192] * 16, 15)]                # |s0 - prvSample| = 8192: a 15-bit delta code, equal to the sub-type-0 code
    w, fired = R.walk(recs, 2, 1, 1)
    assert fired == 1
    assert (w["code"][0, 0], w["sub"][0, 0]) == (0, 1)
    assert (w["code"][0, 1], w["sub"][0, 1]) == (15, 0)
    vals, lens = R.emit(recs, w, 2, 1, 1)
    # band 0: no flag, Invert 0, no samples; band 1: the 0 bit after a zero band, Invert +15, 16 samples of 15 bits
    assert list(lens[:2]) == [0, R.BT_LEN[1, 16]] and not lens[2:17].any()
    assert list(lens[17:19]) == [1, R.BT_LEN[1, 15 + 16]] and list(lens[19:]) == [15] * 16
    # without the carried sub-type 1 (a sub-type-0 band before), Keep is not asked for and the rule stays out
    w, fired = R.walk([_rec([5, -7] + [0] * 13, 4), _rec([8192] * 16, 15)], 2, 1, 1)
    assert fired == 0


def test_delta_codes_from_records_equal_get_delta_band_code():
    """the walk's O(1) delta codes (bit lengths of the in-band deltas and of the two terms with prvSample / prvDelta)
    equal GetDeltaBandCode over buf1 / buf2 computed in full"""
    rng = np.random.default_rng(0xDE17A)

    def direct(buf, typ):
        hi = max(abs(int(buf.min())), abs(int(buf.max())))
        return 0 if hi == 0 else hi.bit_length() + 1 - (1 if typ == 0 else 0)
    for _ in range(2000):
        n = int(rng.choice([15, 16]))
        mag = int(rng.choice([1, 4, 300, 20000]))
        s = rng.integers(-mag, mag + 1, n) * (rng.random() < 0.8)
        P, D = int(rng.integers(-mag, mag + 1)), int(rng.integers(-mag, mag + 1))
        buf1 = np.concatenate([[s[0] - P], np.diff(s)])
        buf2 = np.concatenate([[s[0] - P - D, s[1] - 2 * s[0] + P], np.diff(s, n=2)])
        r = _rec(list(s), 1)
        for typ in (0, 1):
            c1 = R.delta_code(max(abs(int(s[0]) - P).bit_length(), int(r["L1"][0])), typ)
            c2 = R.delta_code(max(abs(int(s[0]) - P - D).bit_length(), abs(int(s[1]) - 2 * int(s[0]) + P).bit_length(), int(r["L2"][0])), typ)
            assert c1 == direct(buf1, typ) and c2 == direct(buf2, typ)
