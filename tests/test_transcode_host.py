"""dcs_transcode_plan (host only) and the transcoding restatement (tests/transcode_ref.py) against the compiled reference.

The plan: EncodeDCSFile's copy-or-re-encode rule for every source OS, type bit, target version and flag, the bytes each
output can take, and the three defined errors.  The restatement: the compiled reference decoder's PCM for the reference's
recipe, through the compiled reference encoder's float path (oracle/_ref/dcs_encref), screened as tests/enc_cases.py
check() screens a case -- a case with a UBSan bounds or float-cast report is dropped, one in which the OS93 Keep +15 rule
fired is held to the restatement -- equals what transcode_ref writes from the oracle's decode."""
import ctypes
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc_cases as C
import enc_ref as E
import transcode_ref as T
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_INVALID_ARG
from util import make_stream

HERE = os.path.dirname(os.path.abspath(__file__))
VERSIONS = [0x9400, 0x9302, 0x9301]
# a layout with the type bit clear and one with it set, per source OS
LAYOUT = {(D.OS93A, 0): D.FMT_93_T0, (D.OS93A, 1): D.FMT_93A_T1, (D.OS93B, 0): D.FMT_93_T0, (D.OS93B, 1): D.FMT_93B_T1,
          (D.OS94, 0): D.FMT_94_T0, (D.OS94, 1): D.FMT_94_T1_S0, (D.OS95, 0): D.FMT_94_T0, (D.OS95, 1): D.FMT_94_T1_S3}
# every target the encoders offer: (version, type, sub-type), -1 = wildcard
TARGETS = [(0x9400, -1, -1), (0x9400, 0, 0), (0x9400, 0, 3), (0x9400, 1, 0), (0x9400, 1, 3),
           (0x9302, -1, -1), (0x9302, 0, -1), (0x9302, 1, -1), (0x9301, 0, -1)]
FAMILY = {0x9400: "94", 0x9302: "93b", 0x9301: "93a"}


def _plan(streams, os_list, version, flags=0, **params):
    """the raw call: (status, actions, bounds)"""
    L = D.load_library()
    p = D.transcode_params(version, **params)
    refs = (D.api.StreamRef * max(1, len(streams)))()
    keep = []
    for k, (s, o) in enumerate(zip(streams, os_list)):
        a = np.frombuffer(bytes(s) + b"\0", dtype=np.uint8)
        keep.append(a)
        refs[k].data, refs[k].len, refs[k].os = a.ctypes.data, len(s), o
        refs[k].volume, refs[k].level, refs[k].channelVolume = 0x67, 0xFF, 0xFF
    action, bound = np.full(max(1, len(streams)), -9, np.int32), np.zeros(max(1, len(streams)), np.uint64)
    st = L.dcs_transcode_plan(refs, len(streams), ctypes.byref(p), flags, D.api._ptr(action), D.api._ptr(bound))
    return st, action[:len(streams)], bound[:len(streams)]


@pytest.mark.parametrize("reencode_all", [False, True])
@pytest.mark.parametrize("version", VERSIONS)
def test_plan_table(version, reencode_all):
    streams, os_list, want_action, want_bound = [], [], [], []
    for (os_, bit), fmt in sorted(LAYOUT.items()):
        s = make_stream(fmt, 20 + 7 * os_ + bit, seed=0x7C0 + 2 * os_ + bit)
        assert (s[2] >> 7) == bit
        a = T.action(s, os_, version, reencode_all)
        # the rule written out once more, by hand
        v = T.VERSION[os_]
        assert a == (T.REENCODED if reencode_all or not (v == version or (v < 0x9400 and version < 0x9400 and bit == 0)) else T.COPIED)
        streams.append(s)
        os_list.append(os_)
        want_action.append(a)
        bound = D.encode_bound if version == 0x9400 else D.encode93_bound
        want_bound.append(len(s) if a == T.COPIED else bound((T.frames(s) + 1) * 240))
    action, bounds = D.transcode_plan(streams, os_list, version, reencode_all=reencode_all)
    assert list(action) == want_action
    assert list(bounds) == want_bound
    # one source at a time: the same
    for s, o, a, b in zip(streams, os_list, want_action, want_bound):
        a1, b1 = D.transcode_plan([s], [o], version, reencode_all=reencode_all)
        assert (a1[0], b1[0]) == (a, b)


def test_plan_copies_every_os93_type0_source_for_either_os93_target():
    s = make_stream(D.FMT_93_T0, 9, seed=3)
    for src in (D.OS93A, D.OS93B):
        for version in (0x9301, 0x9302):
            assert D.transcode_plan([s], [src], version)[0][0] == T.COPIED


def test_plan_errors():
    long93 = bytes([0xFF, 0xFF, 0x80]) + bytes(64)              # 65 535 frames: the plan reads only the count and the type bit
    st, _, _ = _plan([long93], [D.OS93B], 0x9400)
    assert st == ERR_INVALID_ARG
    # ... a copy of it is fine (nothing is decoded or encoded)
    st, a, b = _plan([long93], [D.OS93B], 0x9302)
    assert st == 0 and a[0] == T.COPIED and b[0] == len(long93)
    # 65 534 frames re-encode to 65 535
    st, a, b = _plan([bytes([0xFF, 0xFE, 0x80]) + bytes(64)], [D.OS93B], 0x9400)
    assert st == 0 and a[0] == T.REENCODED and b[0] == D.encode_bound(65535 * 240)
    # OS93a Type 1 has no encoder
    s = make_stream(D.FMT_94_T0, 5, seed=1)
    st, _, _ = _plan([s], [D.OS94], 0x9301, fmt=None, streamFormatType=1)
    assert st == ERR_INVALID_ARG
    # no type bit to read
    for short in (b"", b"\x00", b"\x00\x05"):
        st, _, _ = _plan([s, short], [D.OS94, D.OS94], 0x9400)
        assert st == ERR_BAD_STREAM
    # zero frames, re-encoded
    st, _, _ = _plan([bytes([0, 0, 0x80]) + bytes(16)], [D.OS93B], 0x9400)
    assert st == ERR_BAD_STREAM
    # unknown flags, an unknown OS, an unknown version
    assert _plan([s], [D.OS94], 0x9400, flags=2)[0] == ERR_INVALID_ARG
    assert _plan([s], [7], 0x9400)[0] == ERR_INVALID_ARG
    with pytest.raises(ValueError):
        D.transcode_params(0x9500)


# ---------------------------------------------------------------------------------------------- against the reference
def _case(name, pcm, target):
    version, typ, sub = target
    return C.Case(name, E.to_float(pcm), FAMILY[version], "t%d%d" % (typ, sub), version, typ, sub, dict(E.DEFAULTS))


def _against_reference(reference, oracle, stream, os_, target, name):
    """-> the case's status; asserts the restatement's bytes are the reference composition's"""
    version, typ, sub = target
    ref_pcm = T.decoded(reference, stream, os_)
    assert np.array_equal(ref_pcm, T.decoded(oracle, stream, os_)), name
    mine, a = T.transcode(oracle, stream, os_, version, typ, sub, reencode_all=True)
    assert a == T.REENCODED
    r = C.check(_case(name, ref_pcm, target))
    if r.status == "kept":
        assert mine == r.ref, name
    elif r.status == "rule":
        assert mine == r.want, name
    return r.status


needs_encref = pytest.mark.skipif(not C.reference_available(), reason=C.MISSING)


@needs_encref
def test_restatement_is_the_reference_composition_on_synthetic_sources(reference, oracle):
    statuses = []
    for fmt in range(6):
        s = make_stream(fmt, 24 + 5 * fmt, seed=0x7A5C0 + fmt)
        os_ = D.format_os(fmt)
        for target in TARGETS:
            statuses.append(_against_reference(reference, oracle, s, os_, target, "synth%d->%r" % (fmt, target)))
    assert statuses.count("kept") >= len(statuses) // 2


@needs_encref
def test_restatement_is_the_reference_composition_on_the_recordings(reference, oracle):
    rec = np.load(os.path.join(HERE, "golden", "encoder_golden.npz"))
    names = sorted(k for k in rec.keys() if k.endswith("/stream"))
    assert len(names) == 24
    os_of = {"94": D.OS94, "93b": D.OS93B, "93a": D.OS93A}
    statuses = []
    for k, name in enumerate(names):
        s = rec[name].tobytes()
        statuses.append(_against_reference(reference, oracle, s, os_of[name.split("-")[1]], TARGETS[k % len(TARGETS)], name))
    assert statuses.count("kept") >= len(statuses) // 2
