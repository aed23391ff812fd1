"""The OS93 encoder on the MI355X (dcs_encode93_streams): byte for byte the reference DCSEncoder's OS93 streams
(tests/golden/encode93_golden.*), byte for byte the numpy restatement (tests/enc93_ref.py) on seeded fuzz, independent of
the batch around a stream and of 1994+ calls between, decodable to what the oracle decodes, and loud on bad input."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc93_ref as R
from test_encode93_host import same_as_golden
from test_gpu_encode import _signal

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "encode93_golden.json")))
PCM = np.load(os.path.join(HERE, "golden", "encode_golden.npz"))
LONG = GOLDEN["long"]
OS_OF = {0x9301: D.OS93A, 0x9302: D.OS93B}
FMT_OF = {(0x9301, -1): None, (0x9301, 0): D.FMT_93_T0, (0x9302, -1): None, (0x9302, 0): D.FMT_93_T0, (0x9302, 1): D.FMT_93B_T1}


def _groups(cases):
    """golden cases that share a version, a type and params encode in one batch"""
    out = {}
    for c in cases:
        out.setdefault((c["version"], c["type"], tuple(sorted(c["params"].items()))), []).append(c)
    return out.values()


def test_every_golden_case_is_byte_identical(gpu_ctx):
    cases = [c for c in GOLDEN["cases"] if c["signal"] != LONG["signal"]]
    n = 0
    for group in _groups(cases):
        c0 = group[0]
        streams, info = gpu_ctx.encode93_streams([PCM[c["signal"] + "/pcm"] for c in group], OS_OF[c0["version"]],
                                                 FMT_OF[c0["version"], c0["type"]], **c0["params"])
        for c, s, inf in zip(group, streams, info):
            assert same_as_golden(c, s), c["name"]
            assert (inf["formatType"], inf["formatSubType"]) == (c["winner"], 0), c["name"]
            assert inf["nBytes"] == len(s) and inf["nFrames"] == c["nFrames"]
            n += 1
    assert n == len(cases)


def test_longest_stream_is_the_references(gpu_ctx):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_encode_golden import recording
    case = next(c for c in GOLDEN["cases"] if c["signal"] == LONG["signal"])
    x = recording(LONG["recording"], LONG["frames"])
    streams, info = gpu_ctx.encode93_streams([x], OS_OF[case["version"]], FMT_OF[case["version"], case["type"]], **case["params"])
    assert same_as_golden(case, streams[0])
    assert info[0]["formatType"] == case["winner"] and info[0]["nFrames"] == 65535


def _params(rng):
    return dict(powerBandCutoff=float(np.float32(rng.choice([0.0, 0.8, 0.9, 0.97, 0.995, 1.0]))),
                targetBitRate=int(rng.choice([8000, 24000, 48000, 96000, 128000, 192000, 320000])),
                maximumQuantizationError=float(np.float32(rng.choice([1, 3, 10, 30]) / 32768)))


@pytest.mark.parametrize("seed", range(6))
def test_seeded_fuzz_matches_enc93_ref(gpu_ctx, seed):
    rng = np.random.default_rng(0xF093 + seed)
    version, typ = [(0x9302, -1), (0x9302, 0), (0x9302, 1), (0x9301, 0), (0x9301, -1), (0x9302, 1)][seed]
    p = _params(rng)
    lengths = [int(rng.choice([1, 2, 239, 240, 241, 479, 481])) if k < 8 else int(np.exp(rng.uniform(np.log(240), np.log(240 * 400))))
               for k in range(40)]
    lengths.append(int(rng.integers(240 * 1000, 240 * 1500)))
    pcm = [_signal(rng, n) for n in lengths]
    streams, info = gpu_ctx.encode93_streams(pcm, OS_OF[version], FMT_OF[version, typ], **p)
    for k, (x, s) in enumerate(zip(pcm, streams)):
        want, win, keep, _ = R.encode(x, version, typ, **p)
        assert s == want, (seed, k, len(x))
        assert (info[k]["formatType"], info[k]["formatSubType"], info[k]["bandsToKeep"]) == (win, 0, keep)


def test_batch_invariance(gpu_ctx):
    rng = np.random.default_rng(0xBA793)
    pcm = [_signal(rng, int(rng.integers(1, 240 * 300))) for _ in range(40)]
    together, _ = gpu_ctx.encode93_streams(pcm)
    gpu_ctx.encode_streams(pcm[:5])                     # a 1994+ batch in between shares the context's buffers
    reverse, _ = gpu_ctx.encode93_streams(pcm[::-1])
    assert together == reverse[::-1]
    for k in range(0, 40, 7):
        alone, _ = gpu_ctx.encode93_streams([pcm[k]])
        assert alone[0] == together[k]
        gpu_ctx.encode_streams([pcm[k]])
    t1, _ = gpu_ctx.encode93_streams(pcm, D.OS93B, D.FMT_93B_T1)
    assert [gpu_ctx.encode93_streams([x], D.OS93B, D.FMT_93B_T1)[0][0] for x in pcm[:6]] == t1[:6]


def test_round_trip_through_the_decoder(gpu_ctx, oracle):
    rng = np.random.default_rng(0x2093)
    pcm = [PCM["rec%d/pcm" % v] for v in range(4)] + [_signal(rng, 240 * 50) for _ in range(4)]
    for os_, fmt in [(D.OS93A, D.FMT_93_T0), (D.OS93B, D.FMT_93_T0), (D.OS93B, D.FMT_93B_T1)]:
        streams, _ = gpu_ctx.encode93_streams(pcm, os_, fmt)
        items = [(os_, s, 255, 0x64) for s in streams]
        got, err, first = gpu_ctx.decode_streams(items)
        assert not err.any()
        want = np.concatenate([oracle.decode(os_, 255, [s], [0x64], (s[0] << 8) | s[1]) for s in streams])
        assert np.array_equal(got, want), (os_, fmt)


def test_error_paths(gpu_ctx):
    ok = np.zeros(480, np.float32)
    for bad, status in [([np.zeros(0, np.float32)], -1), ([np.zeros(65535 * 240 + 1, np.float32)], -1),
                        ([ok, np.array([0.1, np.nan], np.float32)], -6), ([np.array([np.inf], np.float32)], -6),
                        ([np.array([0.5, 1.0001], np.float32)], -6)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode93_streams(bad)
        assert e.value.status == status
    # OS93a Type 1: the reference's refusal, with the reason
    with pytest.raises(D.DcsError) as e:
        gpu_ctx.encode93_streams([ok], D.OS93A, D.FMT_93A_T1)
    assert e.value.status == -1 and "OS93a Type 1" in str(e.value)
    for kw in [dict(streamFormatType=2), dict(streamFormatSubType=4), dict(formatVersion=0x9400), dict(targetBitRate=0)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode93_streams([ok], **kw)
        assert e.value.status == -1
    with pytest.raises(D.DcsError) as e:                  # and the 1994+ entry point still refuses OS93
        gpu_ctx.encode_streams([ok], formatVersion=0x9302)
    assert e.value.status == -1
    # capacity: too small an output buffer is refused, with the size needed written out
    from dcsexplorer_amd.api import _encode_input, _ptr
    x, offs = _encode_input([ok, ok])
    p = D.encode93_params(D.OS93B)
    out_offs = np.zeros(3, np.uint64)
    out = np.zeros(8, np.uint8)
    st = gpu_ctx.L.dcs_encode93_streams(gpu_ctx.h, _ptr(x), _ptr(offs), 2, ctypes.byref(p), _ptr(out), 8, _ptr(out_offs), None)
    assert st == -5
    want, _ = gpu_ctx.encode93_streams([ok, ok])
    assert int(out_offs[2]) == sum(len(s) for s in want)
    gpu_ctx.encode93_streams([np.array([1.0, -1.0] * 300, np.float32)])      # exactly 1.0 and -1.0 are in range
