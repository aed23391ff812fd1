"""dcs_flac_parse, dcs_flac_index and dcs_encode_files_plan (host only) against tests/flac_ref.py on the seeded files of
tests/flac_cases.py; the restatement's floats against NyquistIO::Load's in the fixture (tests/golden/flac_golden.*); each
clause of INTEGRATION.md "Encoding files" rules 20-25 that needs no GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import flac_cases as F
import flac_ref as R
import wav_cases as W

CASES = F.cases()
REFUSED = F.refused_cases()
HERE = os.path.dirname(os.path.abspath(__file__))
REF = {c["name"]: c for c in json.load(open(os.path.join(HERE, "golden", "flac_golden.json")))["cases"]}
NPZ = np.load(os.path.join(HERE, "golden", "flac_golden.npz"))


@pytest.mark.parametrize("name,data", CASES, ids=[c[0] for c in CASES])
def test_parse_and_index_match_restatement(name, data):
    got = D.flac_parse(data)
    st, d = R.parse(data)
    assert st == 0 and got["status"] == 0, (name, got["reason"])
    for k, v in d.items():
        assert got[k] == v, (name, k)
    st, frames = D.flac_index(data)
    _, want = R.index(data)
    assert st == 0 and len(frames) == len(want) == got["nFrames"]
    for a, f in zip(frames, want):
        for k, v in f.items():
            assert a[k] == v, (name, int(f["firstSample"]), k)
    # the index covers the file from the first frame on without gaps
    assert frames[0]["offset"] == got["firstFrameOffset"]
    assert all(int(a["offset"]) + int(a["length"]) == int(b["offset"]) for a, b in zip(frames, frames[1:]))


def test_writer_is_deterministic():
    """every recipe gives the bytes the fixture was made from"""
    for name, data in CASES:
        assert hashlib.sha256(data).hexdigest() == REF[name]["file_sha256"], name
    for name, data, _, _, _ in REFUSED:
        assert hashlib.sha256(data).hexdigest() == REF[name]["file_sha256"], name


def test_writer_covers_what_it_says():
    """the shapes the cases are there for, read back through the restatement's walk"""
    seen = dict(types=set(), fixed=set(), lpc=set(), prec_shift=set(), assign=set(), bits=set(), bs_code=set(), rate_code=set(),
                blocking=set(), utf8=set(), wasted=set(), rice=set(), esc=set(), po=set())
    for name, data in CASES:
        st, frames = R.index(data)
        info = R.parse(data)[1]
        seen["bits"].add(info["bitDepth"])
        for f in frames:
            o = f["offset"]
            h = R.header(data, o, info["bitDepth"])
            seen["assign"].add(f["channelAssignment"])
            seen["bs_code"].add(data[o + 2] >> 4)
            seen["rate_code"].add(data[o + 2] & 15)
            seen["blocking"].add(f["blockingStrategy"])
            lead = data[o + 4]
            seen["utf8"].add(1 if lead < 0x80 else 2 if lead < 0xE0 else 3 if lead < 0xF0 else 4)
            if f["blockSize"] > 4096:
                continue
            subs, _ = R.walk(data, o, o + f["length"] - 2, h)
            seen["wasted"].add(tuple(s["wasted"] > 0 for s in subs))
            for s in subs:
                seen["types"].add(s["type"])
                seen["fixed" if s["type"] == "fixed" else "lpc" if s["type"] == "lpc" else "po"].add(s["order"])
    assert seen["types"] == {"const", "verbatim", "fixed", "lpc"} and seen["fixed"] == {0, 1, 2, 3, 4}
    assert {1, 2, 8, 12, 32} <= seen["lpc"]
    assert seen["assign"] == {0, 1, 8, 9, 10} and seen["bits"] == {8, 16, 24} and seen["blocking"] == {0, 1}
    assert seen["bs_code"] == set(range(1, 16)) and seen["rate_code"] == set(range(15))
    assert {1, 2, 3} <= seen["utf8"]
    assert {(True, False), (True, True), (False,)} <= seen["wasted"]


@pytest.mark.parametrize("name,data,status,where,rule", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_cases(name, data, status, where, rule):
    got = D.flac_parse(data)
    st, frames = D.flac_index(data)
    if where == "host":
        assert got["status"] == status and st == status and got["reason"], name
        assert R.parse(data)[0] == status
        if status == R.BAD_STREAM and rule in (21, 23, 24):
            assert got["reason"].startswith("frame "), got["reason"]       # errors name the frame
    else:
        # a kernel refuses it (or the resampler's rate range does): the host index takes it, and the restated walk and
        # restore say what the device will find
        assert got["status"] == 0 and st == 0 and len(frames) == got["nFrames"], (name, got["reason"])
        assert R.integers(data)[0] == (0 if where == "plan" else status)


def test_reasons_of_the_rules():
    by = {c[0]: c[1] for c in REFUSED}
    reason = lambda n: D.flac_parse(by[n])["reason"]
    assert "fLaC" in reason("r20_ogg_flac") and "fLaC" in reason("r20_junk_before_marker")
    assert "bit depth" in reason("r21_bits12") and "bit depth" in reason("r21_bits20")
    assert "channel count" in reason("r21_3ch")
    assert "differs from STREAMINFO" in reason("r21_frame_depth_differs")
    assert "differs from STREAMINFO" in reason("r21_frame_channels_differ")
    assert "total sample count" in reason("r22_total_zero")
    assert "more samples than STREAMINFO" in reason("r22_total_smaller")
    assert "more samples than STREAMINFO" in reason("r22_further_frame")
    assert "CRC-16" in reason("r23_crc16_flipped") and "CRC-16" in reason("r23_crc16_flipped_last")
    assert "negative LPC shift" in reason("r23_negative_lpc_shift_last")
    assert "do not parse" in reason("r23_reserved_subframe_type_last")


def test_restatement_equals_nyquist_load():
    """flac_ref's floats are NyquistIO::Load's: the sha256 over the bits of every accepted case, and the bits themselves
    where the fixture keeps them -- without the library"""
    kept = 0
    for name, data in CASES:
        v = np.asarray(R.values(data), "<f4")
        c = REF[name]
        assert len(v) == c["n_values"], name
        assert hashlib.sha256(v.tobytes()).hexdigest() == c["values_sha256"], name
        if name + "/values" in NPZ:
            assert np.array_equal(v.view(np.uint32), NPZ[name + "/values"].view(np.uint32)), name
            kept += 1
    assert kept >= 15
    v = R.values(dict(CASES)["fullscale_s8_31250"])
    assert v[0] == np.float32(-128) * (np.float32(1) / np.float32(127)) and abs(float(v[0]) + 1.00787401) < 1e-7
    v = R.values(dict(CASES)["fullscale_s16_31250"])
    assert v[0] == np.float32(-32768) / np.float32(32767) and v[1] == 1.0


def test_writer_integers_are_the_restatement_s():
    ints = F.integers()
    for name, data in CASES:
        want, (rate, channels, bits) = ints[name]
        st, x, d = R.integers(data)
        assert st == 0 and np.array_equal(x, R.cut(want, bits)), name
        assert (d["rate"], d["channels"], d["bitDepth"]) == (rate, channels, bits)


def test_reference_loads_every_case_and_screens_clean():
    """what the generator asserted when the fixture was made: every accepted file loads and encodes in the reference, with no
    sanitizer report (rule 25 rests on the full-scale cases among them)"""
    for name, _ in CASES:
        for r in REF[name]["runs"]:
            assert r["load"].startswith("ok") and r["encode"].startswith("ok") and r["ubsan"] == [] and r["rc"] == 0, (name, r)


def test_plan_kinds_and_bounds_in_a_mixed_list():
    by = dict(CASES)
    s = D.synth_stream(D.FMT_94_T0, 20, seed=5)
    container = D.dcsa_header(D.OS94, len(s)) + s
    wav = dict(W.cases())["s16_1ch_22050"]
    files = [by["assign_s16_stereo"], wav, container, by["fullscale_s8_31250"], by["realistic_44100_stereo"], b"OggS" + bytes(60)]
    kind, bound, status = D.encode_files_plan(files)
    assert list(kind) == [D.FILE_FLAC, D.FILE_WAV, D.FILE_DCSA_COPY, D.FILE_FLAC, D.FILE_FLAC, -1]
    assert list(status) == [0, 0, 0, 0, 0, D.api.ERR_INVALID_ARG]
    assert bound[0] == D.encode_bound(D.resample_count(240, 48000, 1))         # 240 mono samples after the downmix
    assert bound[3] == D.encode_bound(240)                                    # 31 250 Hz: passed through
    assert bound[4] == D.encode_bound(D.resample_count(44100, 44100, 1))
    kind93, bound93, _ = D.encode_files_plan(files[:5], version=0x9302)
    assert list(kind93[[0, 3, 4]]) == [D.FILE_FLAC] * 3 and bound93[3] == D.encode93_bound(240)
    # the resampler's rate range and the refusals that need no GPU, in place, with the other files still planned
    ref = {c[0]: c for c in REFUSED}
    kind, _, status = D.encode_files_plan([by["types_s16_mono"], ref["rate_2000_below_range"][1], ref["r22_total_zero"][1],
                                           ref["r21_bits12"][1], ref["r23_reserved_subframe_type"][1]])
    assert list(kind) == [D.FILE_FLAC, -1, -1, -1, D.FILE_FLAC]
    assert list(status) == [0, D.api.ERR_INVALID_ARG, D.api.ERR_BAD_STREAM, D.api.ERR_INVALID_ARG, 0]


def test_wav_parse_still_refuses_flac():
    assert D.wav_parse(CASES[0][1])["status"] == D.api.ERR_INVALID_ARG
    assert D.flac_parse(dict(W.cases())["s16_1ch_22050"])["status"] == D.api.ERR_INVALID_ARG


def test_index_capacity_protocol():
    import ctypes
    from dcsexplorer_amd.api import ERR_CAPACITY, _ptr, load_library
    data = dict(CASES)["frames_300_mono"]
    buf = np.frombuffer(data, np.uint8)
    n = np.zeros(1, np.uint32)
    frames = np.zeros(10, D.FLAC_FRAME_DTYPE)
    assert load_library().dcs_flac_index(_ptr(buf), len(data), _ptr(frames), 10, _ptr(n)) == ERR_CAPACITY
    assert n[0] == 300 and not frames["length"].any()
