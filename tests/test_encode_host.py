"""The 1994+ encoder's host side, without a GPU: the numpy restatement (tests/enc_ref.py) against the reference
encoder's own streams (tests/golden/encode_golden.*), the library's header derivation (dcs_encode_header) against both,
and the size bound."""
import hashlib
import json
import os

import numpy as np
import pytest

import enc_ref as E

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "encode_golden.json")))
ARR = np.load(os.path.join(HERE, "golden", "encode_golden.npz"))
FMT = {"wild": (-1, -1), "T0s0": (0, 0), "T0s3": (0, 3), "T1s0": (1, 0), "T1s3": (1, 3)}
CASES = GOLDEN["cases"]


def same_as_golden(case, s):
    """the reference's stream: its length and sha256, and its bytes where the fixture keeps them"""
    key = case["name"] + "/stream"
    if key in ARR.files and s != ARR[key].tobytes():
        return False
    return len(s) == case["bytes"] and hashlib.sha256(s).hexdigest() == case["sha256"]


def test_golden_covers_the_issue_cases():
    names = {c["name"] for c in CASES}
    for v in range(4):
        assert {"rec%d-%s" % (v, k) for k in FMT} <= names
    for sig in ("len1", "len239", "len240", "len241", "silence", "dc", "square", "noise_fs", "sine40", "near_silent", "float_tones"):
        assert any(c["signal"] == sig for c in CASES), sig
    assert any("shift" in c["ubsan"] for c in CASES)           # the masked-shift rule is exercised
    assert all(set(c["ubsan"]) <= {"shift"} for c in CASES)
    assert sum(c["name"] + "/stream" in ARR.files for c in CASES) >= 30     # small streams kept whole


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_enc_ref_reproduces_the_reference_encoder(case):
    s, win, _ = E.encode(ARR[case["signal"] + "/pcm"], FMT[case["fmt"]], **case["params"])
    assert same_as_golden(case, s)
    assert list(win) == case["winner"]


def _stats(case):
    _, _, _, st = E.analyse_stream(E.to_float(ARR[case["signal"] + "/pcm"]))
    return st


@pytest.mark.parametrize("case", CASES[::3], ids=[c["name"] for c in CASES[::3]])
def test_encode_header_matches_golden_headers(dcs, case):
    ps, lo, hi = _stats(case)
    typ, sub = case["winner"]
    hdr, keep, bits = dcs.encode_header(ps, lo, hi, typ, sub, **case["params"])
    assert hdr.tobytes().hex() == case["header"]
    rh, rk, rb = E.header(ps, lo, hi, typ, sub, dict(E.DEFAULTS, **case["params"]))
    assert keep == rk and list(bits) == list(rb)


def test_encode_header_matches_enc_ref_on_random_statistics(dcs):
    rng = np.random.default_rng(0x4EAD)
    shifts = set()
    for k in range(400):
        scale = 10.0 ** rng.uniform(-8, 1)
        ps = (rng.exponential(1.0, 16) * scale * np.where(rng.random(16) < 0.2, 1e-6, 1.0)).astype(np.float32)
        if k % 7 == 0:
            ps[rng.integers(1, 16):] = 0                          # few bands with power: large shift counts
        lo = (-rng.exponential(0.3, 16)).astype(np.float32)
        hi = rng.exponential(0.3, 16).astype(np.float32)
        p = dict(powerBandCutoff=float(np.float32(rng.choice([0.5, 0.9, 0.97, 0.999, 1.0]))),
                 targetBitRate=int(rng.choice([1000, 8000, 32000, 128000, 256000, 1000000])))
        for typ, sub in E.VARIANTS:
            hdr, keep, bits = dcs.encode_header(ps, lo, hi, typ, sub, **p)
            rh, rk, rb = E.header(ps, lo, hi, typ, sub, dict(E.DEFAULTS, **p))
            assert hdr.tobytes() == rh.tobytes() and keep == rk and list(bits) == list(rb), (k, typ, sub)
            shifts.update(int(b) for b in bits[:keep])
    assert max(shifts) >= 32


def test_encode_bound_bounds_every_golden_stream(dcs):
    for c in CASES:
        n = len(ARR[c["signal"] + "/pcm"])
        assert c["bytes"] <= dcs.encode_bound(n)
    assert dcs.encode_bound(0) == 0 and dcs.encode_bound(65535 * 240) > 0 and dcs.encode_bound(65535 * 240 + 1) == 0


def test_encode_params_default_are_the_references(dcs):
    import ctypes
    p = dcs.EncodeParams()
    assert dcs.load_library().dcs_encode_params_default(ctypes.byref(p)) == 0
    assert (p.formatVersion, p.streamFormatType, p.streamFormatSubType, p.targetBitRate) == (0x9400, 1, 3, 128000)
    assert p.powerBandCutoff == np.float32(0.97) and p.minimumDynamicRange == np.float32(10 / 32768)
    assert p.maximumQuantizationError == np.float32(10 / 32768)


def test_encode_header_rejects_bad_arguments(dcs):
    z = np.zeros(16, np.float32)
    for typ, sub, kw in [(2, 0, {}), (0, 1, {}), (1, 3, dict(targetBitRate=0)), (1, 3, dict(formatVersion=0x9302))]:
        with pytest.raises(dcs.DcsError) as e:
            dcs.encode_header(z, z, z, typ, sub, **kw)
        assert e.value.status == -1


def test_encoder_functions_are_exported(dcs):
    from dcsexplorer_amd.api import EXPORTS
    L = dcs.load_library()
    for name in ("dcs_encode_params_default", "dcs_encode_bound", "dcs_encode_header", "dcs_encode_streams"):
        assert name in EXPORTS and hasattr(L, name)
