"""The OS93a Type-1 encoder on the MI355X (dcs_encode93a_streams): bytes and both info records equal to the numpy
restatement's (tests/enc93a_ref.py, itself held to the compiled reference decoder by tests/test_encode93a_host.py),
independent of the batch around a stream, Type 0 equal to dcs_encode93_streams, decodable by the library's own decoder to
what the reference decodes, and loud on bad input."""
import ctypes

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc93a_cases as C
import enc93a_ref as A

pytestmark = pytest.mark.gpu

FMT = {1: D.FMT_93A_T1, 0: D.FMT_93_T0, -1: None}
SETS = [(rate, mqe, typ) for rate in C.RATES for mqe in C.MQES for typ in C.TYPES]


def _check(name, got, inf, infa, want):
    s, typ, keep, ch = want
    assert got == s, name
    assert (inf["formatType"], inf["formatSubType"], inf["nBytes"], inf["bandsToKeep"]) == (typ, 0, len(s), keep), name
    assert inf["nFrames"] == (s[0] << 8 | s[1])
    assert [int(infa[k]) for k in ("selector", "ladderIndex", "numBands", "frameBits", "budgetBits", "sqErr")] == \
        [ch[k] for k in ("selector", "ladderIndex", "numBands", "frameBits", "budgetBits", "sqErr")], name


@pytest.mark.parametrize("rate,mqe,typ", SETS, ids=["%d-%s-%s" % (r, "q0" if q == 0 else "qd", "t1" if t == 1 else "any") for r, q, t in SETS])
def test_every_case_equals_the_restatement(gpu_ctx, rate, mqe, typ):
    streams, info, infa = gpu_ctx.encode93a_streams([C.SIGNALS[n] for n in C.NAMES], FMT[typ], **C.params(rate, mqe))
    for k, name in enumerate(C.NAMES):
        _check(name, streams[k], info[k], infa[k], C.expected(name, rate, mqe, typ))


def test_batch_invariance(gpu_ctx):
    rng = np.random.default_rng(0xBA93A)
    pcm = [C.SIGNALS[n] for n in C.NAMES]
    alone = [gpu_ctx.encode93a_streams([x], D.FMT_93A_T1)[0][0] for x in pcm]
    order = rng.permutation(len(pcm))
    together, _, _ = gpu_ctx.encode93a_streams([pcm[k] for k in order], D.FMT_93A_T1)
    assert [together[list(order).index(k)] for k in range(len(pcm))] == alone
    wild, info, _ = gpu_ctx.encode93a_streams([pcm[k] for k in order])
    assert [wild[list(order).index(k)] for k in range(len(pcm))] == [gpu_ctx.encode93a_streams([x])[0][0] for x in pcm]
    assert {int(t) for t in info["formatType"]} <= {0, 1}


def test_type0_is_encode93_streams(gpu_ctx):
    pcm = [C.SIGNALS[n] for n in C.NAMES]
    for p in (dict(), C.params(8000, 0.0)):
        got, info, infa = gpu_ctx.encode93a_streams(pcm, D.FMT_93_T0, **p)
        want, winfo = gpu_ctx.encode93_streams(pcm, D.OS93A, D.FMT_93_T0, **p)
        assert got == want and np.array_equal(info, winfo) and not infa["frameBits"].any()


def test_round_trip_through_the_decoder(gpu_ctx, reference):
    names = [n for n in C.NAMES if n.startswith("rec:")] + ["noise_fs", "sine100_fs", "tone_band17"]
    streams, info, _ = gpu_ctx.encode93a_streams([C.SIGNALS[n] for n in names], D.FMT_93A_T1)
    assert (info["formatType"] == 1).all()
    items = [(D.OS93A, s, 255, 0xFF) for s in streams]
    got, err, first = gpu_ctx.decode_streams(items)
    assert not err.any()
    want = np.concatenate([reference.decode(D.OS93A, 255, [s], [0xFF], (s[0] << 8) | s[1]) for s in streams])
    assert np.array_equal(got, want)
    # two such streams on one decoder object: the second starts in what the first's level left behind
    a, b = streams[0], streams[-2]
    got, err, first = gpu_ctx.decode_stream_sequence(D.OS93A, 255, [a, b], [0x64, 0x50], extra_frames=2)
    assert not err.any() and first[-1] == got.shape[0]
    assert np.array_equal(got, reference.decode_sequence(D.OS93A, 255, [a, b], [0x64, 0x50], 2))


def test_error_paths(gpu_ctx):
    ok = np.zeros(480, np.float32)
    for bad, status in [([np.zeros(0, np.float32)], -1), ([np.zeros(65535 * 240 + 1, np.float32)], -1),
                        ([ok, np.array([0.1, np.nan], np.float32)], -6), ([np.array([np.inf], np.float32)], -6),
                        ([np.array([0.5, 1.0001], np.float32)], -6)]:
        for fmt in (D.FMT_93A_T1, None):
            with pytest.raises(D.DcsError) as e:
                gpu_ctx.encode93a_streams(bad, fmt)
            assert e.value.status == status
    for kw in [dict(streamFormatType=2), dict(streamFormatSubType=4), dict(formatVersion=0x9400), dict(formatVersion=0x9302),
               dict(targetBitRate=0)]:
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.encode93a_streams([ok], D.FMT_93A_T1, **kw)
        assert e.value.status == -1
    with pytest.raises(D.DcsError) as e:                  # the OS93 entry point keeps its refusal
        gpu_ctx.encode93_streams([ok], D.OS93A, D.FMT_93A_T1)
    assert e.value.status == -1 and "OS93a Type 1" in str(e.value)
    # capacity: too small an output buffer is refused, with the size needed written out
    from dcsexplorer_amd.api import _encode_input, _ptr
    x, offs = _encode_input([ok, C.SIGNALS["noise_fs"]])
    for typ in (1, -1):
        p = D.encode_params(None, formatVersion=0x9301, streamFormatType=typ, streamFormatSubType=-1)
        out_offs = np.zeros(3, np.uint64)
        out = np.zeros(8, np.uint8)
        st = gpu_ctx.L.dcs_encode93a_streams(gpu_ctx.h, _ptr(x), _ptr(offs), 2, ctypes.byref(p), _ptr(out), 8, _ptr(out_offs), None, None)
        assert st == -5
        want, _, _ = gpu_ctx.encode93a_streams([ok, C.SIGNALS["noise_fs"]], D.FMT_93A_T1 if typ == 1 else None)
        assert int(out_offs[2]) == sum(len(s) for s in want) and not out.any()
    gpu_ctx.encode93a_streams([np.array([1.0, -1.0] * 300, np.float32)], D.FMT_93A_T1)      # exactly 1.0 and -1.0 are in range


def test_300_frames_of_noise(gpu_ctx):
    rng = np.random.default_rng(0x300A)
    x = (rng.standard_normal(240 * 300) * 0.2).clip(-1, 1).astype(np.float32)
    streams, info, infa = gpu_ctx.encode93a_streams([x, C.SIGNALS["dc"]], D.FMT_93A_T1, targetBitRate=96000)
    s, ch, _ = A.encode_type1(A.analyse(x), targetBitRate=96000)
    assert streams[0] == s and int(infa[0]["sqErr"]) == ch["sqErr"] and int(infa[0]["frameBits"]) == ch["frameBits"]
    assert info[0]["nFrames"] == 300 and ch["fits"]
