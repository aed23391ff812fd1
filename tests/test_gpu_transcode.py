"""dcs_transcode_streams on the MI355X: byte for byte the transcoding composition (tests/transcode_ref.py: the oracle's decode
for the reference's recipe, / 32768, the encoder restatements), and the compiled reference's composition where oracle/_ref is
built; copies verbatim; independent of the batch around a stream; decodable to what the oracle decodes; loud on bad input."""
import ctypes

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc_cases as C
import enc_ref as E
import transcode_ref as T
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_CAPACITY, ERR_INVALID_ARG
from oracle.dcs_oracle import Reference, reference_available
from test_transcode_host import FAMILY, TARGETS
from util import corrupt, make_stream

pytestmark = pytest.mark.gpu

# a target (version, type, sub-type) -> the fmt argument of transcode_streams
FMT = {(0x9400, -1, -1): None, (0x9400, 0, 0): D.FMT_94_T0, (0x9400, 0, 3): D.FMT_94_T0_S3, (0x9400, 1, 0): D.FMT_94_T1_S0,
       (0x9400, 1, 3): D.FMT_94_T1_S3, (0x9302, -1, -1): None, (0x9302, 0, -1): D.FMT_93_T0, (0x9302, 1, -1): D.FMT_93B_T1,
       (0x9301, 0, -1): D.FMT_93_T0}


def _sources(seed, nframes=None):
    """one stream of every unpack layout, with the OS it plays under"""
    out = []
    for fmt in range(6):
        n = nframes or 17 + 6 * fmt
        out.append((make_stream(fmt, n, seed=seed + fmt), D.format_os(fmt, prefer_95=bool(seed & 1), prefer_93a=bool(seed & 1))))
    return out


def _want(oracle, s, os_, target, reencode_all=False, **params):
    version, typ, sub = target
    return T.transcode(oracle, s, os_, version, typ, sub, reencode_all, **params)


def _call(ctx, srcs, target, reencode_all=False, **params):
    return ctx.transcode_streams([s for s, _ in srcs], [o for _, o in srcs], target[0], FMT[target], reencode_all, **params)


@pytest.mark.parametrize("reencode_all", [False, True])
@pytest.mark.parametrize("target", TARGETS, ids=lambda t: "%x-%d-%d" % t)
def test_every_layout_into_every_target(gpu_ctx, oracle, target, reencode_all):
    srcs = _sources(0x7A0 + 16 * TARGETS.index(target))
    out, info = _call(gpu_ctx, srcs, target, reencode_all)
    ref = Reference() if reference_available() and C.reference_available() else None
    for k, ((s, os_), got, inf) in enumerate(zip(srcs, out, info)):
        want, action = _want(oracle, s, os_, target, reencode_all)
        assert inf["action"] == action and inf["srcFrames"] == T.frames(s)
        assert got == want, (k, target)
        assert inf["enc"]["nBytes"] == len(got)
        if action == T.COPIED:
            assert got == s and inf["enc"]["bandsToKeep"] == -1 and inf["enc"]["nFrames"] == T.frames(s)
            continue
        assert inf["enc"]["nFrames"] == T.frames(s) + 1 and T.frames(got) == T.frames(s) + 1
        if ref is not None:
            # the compiled reference's composition: its decoder's PCM through its encoder's float path
            pcm = T.decoded(ref, s, os_)
            r = C.check(C.Case("t%d" % k, E.to_float(pcm), FAMILY[target[0]], "x", target[0], target[1], target[2], dict(E.DEFAULTS)))
            if r.status == "kept":
                assert got == r.ref, (k, target)


def test_copies_are_verbatim(gpu_ctx):
    # for 0x9302: an OS93b stream of either type and an OS93a Type-0 stream; trailing bytes past the stream are copied as well
    srcs = [(make_stream(D.FMT_93B_T1, 30, seed=1), D.OS93B), (make_stream(D.FMT_93_T0, 30, seed=2), D.OS93B),
            (make_stream(D.FMT_93_T0, 30, seed=3), D.OS93A), (make_stream(D.FMT_93B_T1, 12, seed=4) + b"\x5a" * 7, D.OS93B)]
    out, info = gpu_ctx.transcode_streams([s for s, _ in srcs], [o for _, o in srcs], 0x9302)
    assert out == [s for s, _ in srcs]
    assert list(info["action"]) == [T.COPIED] * 4
    assert list(info["enc"]["formatType"]) == [1, 0, 0, 1]


@pytest.mark.parametrize("seed", [0, 0x5EED])
def test_mixed_batch_equals_per_stream_calls(gpu_ctx, oracle, seed):
    # families interleaved, copies and re-encodes interleaved, two targets
    srcs = [x for pair in zip(_sources(0x1000), _sources(0x2001)) for x in pair]
    for target in [(0x9400, -1, -1), (0x9302, -1, -1)]:
        try:
            gpu_ctx.set_test_hooks(chunk_order_seed=seed)
            out, info = _call(gpu_ctx, srcs, target)
        finally:
            gpu_ctx.set_test_hooks(0)
        actions = list(info["action"])
        assert T.COPIED in actions and T.REENCODED in actions
        for (s, os_), got in zip(srcs, out):
            one, _ = _call(gpu_ctx, [(s, os_)], target)
            assert got == one[0]
            assert got == _want(oracle, s, os_, target)[0]


def test_reencode_all_shrinks_at_a_lower_rate(gpu_ctx, oracle):
    srcs = [(make_stream(fmt, 40, seed=0x77 + fmt), D.OS94) for fmt in (D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3)]
    target = (0x9400, -1, -1)
    same, info = _call(gpu_ctx, srcs, target)
    assert same == [s for s, _ in srcs] and not info["action"].any()
    out, info = _call(gpu_ctx, srcs, target, True, targetBitRate=32000)
    assert list(info["action"]) == [T.REENCODED] * 3
    for (s, os_), got in zip(srcs, out):
        assert got == _want(oracle, s, os_, target, True, targetBitRate=32000)[0]
        assert len(got) <= len(s)


def test_round_trip_through_the_decoder(gpu_ctx, oracle):
    srcs = _sources(0x3300)
    for target in [(0x9400, -1, -1), (0x9302, -1, -1), (0x9301, 0, -1)]:
        out, info = _call(gpu_ctx, srcs, target, True)
        tos = D.TRANSCODE_OS[target[0]]
        for (s, os_), got in zip(srcs, out):
            want = _want(oracle, s, os_, target, True)[0]
            pcm, err, _ = gpu_ctx.decode_streams([(tos, got, 0x67, 0xFF)], extra_frames=2)
            assert not err.any()
            assert np.array_equal(pcm, oracle.decode(tos, 0x67, [want], [0xFF], T.frames(want) + 2))


def test_dcsa_containers(gpu_ctx, oracle):
    srcs = _sources(0x4400)
    boxes = [D.dcsa_header(os_, len(s)) + s for s, os_ in srcs]
    out, info = gpu_ctx.transcode_dcsa(boxes, 0x9302)
    for (s, os_), box in zip(srcs, out):
        os2, body = D.dcsa_parse(box)
        assert os2 == D.OS93B and box[:36] == D.dcsa_header(D.OS93B, len(body))
        # the container does not tell OS95 from OS94
        assert body == _want(oracle, s, D.OS94 if os_ == D.OS95 else os_, (0x9302, -1, -1))[0]


def test_longest_source(gpu_ctx, oracle):
    s = make_stream(D.FMT_94_T1_S0, 65534, seed=0x10E6)
    target = (0x9301, 0, -1)
    out, info = _call(gpu_ctx, [(s, D.OS94)], target)
    assert info[0]["enc"]["nFrames"] == 65535 and T.frames(out[0]) == 65535
    assert out[0] == _want(oracle, s, D.OS94, target)[0]
    too_long = make_stream(D.FMT_94_T1_S0, 65535, seed=0x10E7)
    with pytest.raises(D.DcsError) as e:
        _call(gpu_ctx, [(s, D.OS94), (too_long, D.OS94)], target)
    assert e.value.status == ERR_INVALID_ARG and "stream 1" in str(e.value)


def _bad_source():
    """a corrupted stream whose decode reports an error word (the index pass stops it early)"""
    base = make_stream(D.FMT_94_T1_S0, 40, seed=0xBAD)
    for seed in range(1, 200):
        s = corrupt(base, seed, nflips=6)
        _, inf = D.index_stream(D.OS94, s)
        if inf.nValidFrames < inf.nFrames:
            return s
    raise AssertionError("no corruption seed stops the stream")


def test_decode_error_is_bad_stream(gpu_ctx):
    bad = _bad_source()
    _, err, _ = gpu_ctx.decode_streams([(D.OS94, bad, 0x67, 0xFF)], extra_frames=1)
    assert err.any()
    good = make_stream(D.FMT_93B_T1, 20, seed=5)
    with pytest.raises(D.DcsError) as e:
        gpu_ctx.transcode_streams([good, good, bad], [D.OS93B, D.OS93B, D.OS94], 0x9302, reencode_all=True)
    assert e.value.status == ERR_BAD_STREAM and "stream 2" in str(e.value)
    # the same source is copied without a look inside
    out, _ = gpu_ctx.transcode_streams([bad], [D.OS94], 0x9400)
    assert out == [bad]
    # and the context still works
    out, _ = gpu_ctx.transcode_streams([good], [D.OS93B], 0x9400)
    assert T.frames(out[0]) == 21


def test_truncated_source_decodes_as_decode_streams(gpu_ctx):
    # bytes past the end read as zero, as dcs_decode_streams reads them (the device planner cannot serve such a list: the
    # host-planned batch decodes it)
    full = make_stream(D.FMT_93B_T1, 60, seed=0x7E)
    s = full[:len(full) // 2]
    pcm, err, _ = gpu_ctx.decode_streams([(D.OS93B, s, 0x67, 0xFF)], extra_frames=1)
    if err.any():
        with pytest.raises(D.DcsError) as e:
            gpu_ctx.transcode_streams([s], [D.OS93B], 0x9400)
        assert e.value.status == ERR_BAD_STREAM
    else:
        out, _ = gpu_ctx.transcode_streams([s], [D.OS93B], 0x9400)
        assert out == gpu_ctx.encode_streams([pcm.ravel()])[0]


def test_capacity_fills_the_offsets(gpu_ctx, oracle):
    srcs = _sources(0x5500)
    want, _ = _call(gpu_ctx, srcs, (0x9400, -1, -1))
    L = D.load_library()
    p = D.transcode_params(0x9400)
    keep = [np.frombuffer(s, np.uint8) for s, _ in srcs]
    refs = (D.api.StreamRef * len(srcs))()
    for k, (s, os_) in enumerate(srcs):
        refs[k].data, refs[k].len, refs[k].os = keep[k].ctypes.data, len(s), os_
        refs[k].volume, refs[k].level, refs[k].channelVolume = 0x67, 0xFF, 0xFF
    total = sum(len(x) for x in want)
    out = np.zeros(total, np.uint8)
    offs = np.zeros(len(srcs) + 1, np.uint64)
    st = L.dcs_transcode_streams(gpu_ctx.h, refs, len(srcs), ctypes.byref(p), 0, D.api._ptr(out), total - 1, D.api._ptr(offs), None)
    assert st == ERR_CAPACITY
    assert list(np.diff(offs)) == [len(x) for x in want]
    st = L.dcs_transcode_streams(gpu_ctx.h, refs, len(srcs), ctypes.byref(p), 0, D.api._ptr(out), total, D.api._ptr(offs), None)
    assert st == 0 and out.tobytes() == b"".join(want)
