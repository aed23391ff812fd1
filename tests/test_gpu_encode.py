"""The 1994+ encoder on the MI355X (dcs_encode_streams): byte for byte the reference DCSEncoder's streams
(tests/golden/encode_golden.*), byte for byte the numpy restatement (tests/enc_ref.py) on seeded fuzz, independent of
the batch around a stream, decodable to what the oracle decodes, and loud on bad input."""
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc_ref as E
from test_encode_host import same_as_golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "encode_golden.json")))["cases"]
ARR = np.load(os.path.join(HERE, "golden", "encode_golden.npz"))
FMT = {"wild": None, "T0s0": D.FMT_94_T0, "T0s3": D.FMT_94_T0_S3, "T1s0": D.FMT_94_T1_S0, "T1s3": D.FMT_94_T1_S3}
REF_FMT = {None: (-1, -1), D.FMT_94_T0: (0, 0), D.FMT_94_T0_S3: (0, 3), D.FMT_94_T1_S0: (1, 0), D.FMT_94_T1_S3: (1, 3)}


def _groups(cases):
    """golden cases that share a layout and params encode in one batch"""
    out = {}
    for c in cases:
        out.setdefault((c["fmt"], tuple(sorted(c["params"].items()))), []).append(c)
    return out.values()


def test_every_golden_case_is_byte_identical(gpu_ctx):
    n = 0
    for group in _groups(GOLDEN):
        streams, info = gpu_ctx.encode_streams([ARR[c["signal"] + "/pcm"] for c in group], FMT[group[0]["fmt"]], **group[0]["params"])
        for c, s, inf in zip(group, streams, info):
            assert same_as_golden(c, s), c["name"]
            assert [inf["formatType"], inf["formatSubType"]] == c["winner"], c["name"]
            assert inf["nBytes"] == len(s) and inf["nFrames"] == c["nFrames"]
            n += 1
    assert n == len(GOLDEN)


def _signal(rng, n):
    t = np.arange(n) / 31250.0
    kind = rng.integers(0, 6)
    if kind == 0:
        x = sum(rng.uniform(0, 0.4) * np.sin(2 * np.pi * rng.uniform(20, 15000) * t + rng.uniform(0, 6)) for _ in range(rng.integers(1, 5)))
    elif kind == 1:
        x = rng.uniform(-1, 1) * rng.uniform(0, 1) * np.ones(n)
    elif kind == 2:
        x = np.zeros(n)
    else:
        x = rng.normal(0, rng.uniform(1e-4, 0.5), n)
        x += 0.3 * np.sin(2 * np.pi * rng.uniform(30, 4000) * t)
    if rng.random() < 0.3:                                  # silent stretch
        a = rng.integers(0, n)
        x[a:a + rng.integers(0, n)] = 0
    if rng.random() < 0.3:                                  # clipping
        x *= rng.uniform(1, 4)
    x = np.clip(x, -1, 1)
    if rng.random() < 0.5:
        return np.clip(np.rint(x * 32767), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


def _params(rng):
    return dict(powerBandCutoff=float(np.float32(rng.choice([0.8, 0.9, 0.97, 0.995, 1.0]))),
                targetBitRate=int(rng.choice([24000, 48000, 96000, 128000, 192000, 320000])),
                minimumDynamicRange=float(np.float32(rng.choice([0, 2, 10, 40]) / 32768)),
                maximumQuantizationError=float(np.float32(rng.choice([2, 6, 10, 30]) / 32768)))


@pytest.mark.parametrize("seed", range(6))
def test_seeded_fuzz_matches_enc_ref(gpu_ctx, seed):
    rng = np.random.default_rng(0xF022 + seed)
    fmt = [None, D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3, D.FMT_94_T0_S3, None][seed]
    p = _params(rng)
    lengths = [int(rng.choice([1, 2, 239, 240, 241, 479, 481])) if k < 8 else int(np.exp(rng.uniform(np.log(240), np.log(240 * 600))))
               for k in range(52)]
    lengths.append(int(rng.integers(240 * 2000, 240 * 3000)))
    if seed == 0:
        lengths.append(240 * 20000 + 17)                   # one long stream
    pcm = [_signal(rng, n) for n in lengths]
    streams, info = gpu_ctx.encode_streams(pcm, fmt, **p)
    for k, (x, s) in enumerate(zip(pcm, streams)):
        want, win, keep = E.encode(x, REF_FMT[fmt], **p)
        assert s == want, (seed, k, len(x))
        assert (info[k]["formatType"], info[k]["formatSubType"]) == win and info[k]["bandsToKeep"] == keep


def test_batch_invariance(gpu_ctx):
    rng = np.random.default_rng(0xBA7C)
    pcm = [_signal(rng, int(rng.integers(1, 240 * 300))) for _ in range(40)]
    together, _ = gpu_ctx.encode_streams(pcm)
    reverse, _ = gpu_ctx.encode_streams(pcm[::-1])
    assert together == reverse[::-1]
    for k in range(0, 40, 7):
        alone, _ = gpu_ctx.encode_streams([pcm[k]])
        assert alone[0] == together[k]


def test_round_trip_through_the_decoder(gpu_ctx, oracle):
    rng = np.random.default_rng(0x2071)
    pcm = [ARR["rec%d/pcm" % v] for v in range(4)] + [_signal(rng, 240 * 50) for _ in range(4)]
    for fmt, os_ in [(D.FMT_94_T0, D.OS94), (D.FMT_94_T0_S3, D.OS95), (D.FMT_94_T1_S0, D.OS94), (D.FMT_94_T1_S3, D.OS95)]:
        streams, _ = gpu_ctx.encode_streams(pcm, fmt)
        items = [(os_, s, 255, 0x64) for s in streams]
        got, err, first = gpu_ctx.decode_streams(items)
        assert not err.any()
        want = np.concatenate([oracle.decode(os_, 255, [s], [0x64], (s[0] << 8) | s[1]) for s in streams])
        assert np.array_equal(got, want), fmt


def test_error_paths(gpu_ctx):
    ok = np.zeros(480, np.float32)
    for bad, status in [([np.zeros(0, np.float32)], -1), ([np.zeros(65535 * 240 + 1, np.float32)], -1),
                        ([ok, np.array([0.1, np.nan], np.float32)], -6), ([np.array([np.inf], np.float32)], -6),
                        ([np.array([0.5, 1.0001], np.float32)], -6)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_streams(bad)
        assert e.value.status == status
    for kw in [dict(streamFormatType=2), dict(streamFormatSubType=1), dict(formatVersion=0x9302), dict(targetBitRate=0)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode_streams([ok], **kw)
        assert e.value.status == -1
    # capacity: too small an output buffer is refused, with the size needed written out
    import ctypes
    from dcsexplorer_amd.api import _encode_input, _ptr
    x, offs = _encode_input([ok, ok])
    p = D.encode_params()
    out_offs = np.zeros(3, np.uint64)
    out = np.zeros(8, np.uint8)
    st = gpu_ctx.L.dcs_encode_streams(gpu_ctx.h, _ptr(x), _ptr(offs), 2, ctypes.byref(p), _ptr(out), 8, _ptr(out_offs), None)
    assert st == -5
    want, _ = gpu_ctx.encode_streams([ok, ok])
    assert int(out_offs[2]) == sum(len(s) for s in want)
    # exactly 1.0 and -1.0 are in range
    gpu_ctx.encode_streams([np.array([1.0, -1.0] * 300, np.float32)])
