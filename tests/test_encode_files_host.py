"""dcs_wav_parse and dcs_encode_files_plan (host only) against tests/wav_ref.py on the seeded cases of tests/wav_cases.py,
and each numbered rule of INTEGRATION.md "Encoding files" that needs no GPU."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import dcsexplorer_amd as D
import wav_cases as W
import wav_ref as R

CASES = W.cases()
EDGE = W.float_edge_cases()
REF = {c["name"]: c for c in json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                                           "encode_file_golden.json")))["cases"]}


@pytest.mark.parametrize("name,data", CASES, ids=[c[0] for c in CASES])
def test_parse_matches_restatement(name, data):
    got = D.wav_parse(data)
    st, d = R.parse(data)
    assert got["status"] == st, (name, got["reason"])
    assert (st == 0) == (not name.startswith("err_")), name
    if st != 0:
        assert got["reason"]
        return
    for k in ("formatCode", "channels", "rate", "blockAlign", "bitDepth", "sampleFormat", "dataOffset", "dataSize", "nValues"):
        assert got[k] == d[k], (name, k)


def test_statuses_of_the_refusals():
    by = dict(CASES)
    want = {
        "err_size_63": R.INVALID_ARG, "err_riff_size": R.INVALID_ARG, "err_rifx": R.INVALID_ARG, "err_mulaw": R.INVALID_ARG,
        "err_3ch": R.INVALID_ARG, "err_bits12": R.INVALID_ARG, "err_int64": R.INVALID_ARG, "err_ext_other": R.INVALID_ARG,
        "err_no_data": R.INVALID_ARG, "err_blockalign0": R.BAD_STREAM, "err_data_past_end": R.BAD_STREAM,
        "err_fmt_at_end": R.BAD_STREAM, "err_ima_reserved": R.BAD_STREAM, "err_ima_no_fact": R.BAD_STREAM,
        "err_ima_step89": R.BAD_STREAM, "err_ima_overflow": R.BAD_STREAM,
    }
    for name, st in want.items():
        assert D.wav_parse(by[name])["status"] == st, name
    assert "big-endian" in D.wav_parse(by["err_rifx"])["reason"]
    assert D.wav_parse(by["size_64"])["status"] == 0


def test_scan_takes_data_inside_list():
    """ScanForChunk finds the first 2-byte-aligned 'data' anywhere: the one inside the LIST payload (rule 8)"""
    b = dict(CASES)["scan_trap_data_in_list"]
    got = D.wav_parse(b)
    assert got["status"] == 0
    list_at = b.index(b"LIST")
    assert got["dataOffset"] == list_at + 8 + 4 + 8 and got["dataSize"] == 64
    assert got["nValues"] == 32


def test_extensible_float_is_read_as_float():
    """rule 10: EXTENSIBLE with the IEEE float sub-format is float (libnyquist would read it as int32)"""
    b = dict(CASES)["ext_float_f32"]
    got = D.wav_parse(b)
    assert got["formatCode"] == 0xFFFE and got["sampleFormat"] == D.WAV_F32
    v = R.values(b, R.parse(b)[1])
    assert np.array_equal(v, W.signal("f32", 2400, 6).astype(np.float32))
    assert D.wav_parse(dict(CASES)["ext_pcm_s32"])["sampleFormat"] == D.WAV_S32


def test_conversion_constants():
    """the *_to_float32 expressions, bit for bit: int16 / 32767, u8 (s - 128) * (1/127), s24 / 2^23, s32 / 2^31"""
    i16 = np.arange(-32768, 32768, dtype=np.int64)
    b = W.wav("s16", 1, 8000, i16)
    v = R.values(b, R.parse(b)[1])
    assert v[0] == np.float32(-32768) / np.float32(32767) and v[-1] == 1.0
    assert v[0] < -1.0                                      # full-scale negative: -1.0000305
    u8 = np.arange(256)
    b = W.wav("u8", 1, 8000, u8)
    v = R.values(b, R.parse(b)[1])
    assert v[128] == 0.0 and abs(float(v[0]) + 1.0078740) < 1e-6


def test_downmix_keeps_the_unpaired_value():
    v = np.array([0.5, 0.25, -0.5, 0.125, 0.75], np.float32)
    assert np.array_equal(R.downmix(v, 2), np.array([0.375, -0.1875, 0.75], np.float32))


def test_ima_wraps_instead_of_clamping():
    """int16_t p += diff wraps (x86 g++): 32700 + 61 436 is 28 600, where a clamp would give 32 767"""
    b = W.ima_wrap_wav()                                    # nibble 7: + (step + step/2 + step/4 + step/8)
    st, d = R.parse(b)
    assert st == 0 and D.wav_parse(b)["status"] == 0
    x = R.ima_decode(b, d)
    assert x[0] == 32700 + 61436 - 65536


def test_plan_kinds_and_bounds():
    s = D.synth_stream(D.FMT_94_T0, 30, seed=5)
    container = D.dcsa_header(D.OS94, len(s)) + s
    files = [dict(CASES)["s16_2ch_44100"], container, b"not a file at all, just some bytes" * 3]
    kind, bound, status = D.encode_files_plan(files)
    assert list(kind[:2]) == [D.FILE_WAV, D.FILE_DCSA_COPY] and kind[2] == -1
    assert status[0] == 0 and status[1] == 0 and status[2] == R.INVALID_ARG
    assert bound[1] == len(s)
    st, d = R.parse(files[0])
    assert bound[0] >= D.encode_bound(D.resample_count(d["nValues"], 44100, 2))
    kind, bound, status = D.encode_files_plan([container], version=0x9302)
    assert kind[0] == D.FILE_DCSA_REENCODE
    kind, bound, status = D.encode_files_plan([dict(CASES)["enc_err_rate_low"], dict(CASES)["err_ima_step89"]])
    assert list(status) == [R.INVALID_ARG, R.BAD_STREAM] and list(kind) == [-1, -1]


def test_long_file_recipe():
    b = W.long_wav(seconds=1)
    st, d = R.parse(b)
    assert st == 0 and d["nValues"] == 2 * 44100 and d["channels"] == 2


def test_length_limit_before_allocation():
    """a 316-byte ADPCM file whose fact chunk claims 4 294 967 280 values parses, as libnyquist reads it, but the plan refuses
    it before anything is allocated: fewer than 2^31 mono samples, and a length the encoder could take"""
    b = W.ima_huge_fact_wav()
    assert len(b) < 400
    got = D.wav_parse(b)
    assert got["status"] == 0 and got["nValues"] == 0xFFFFFFF0
    kind, bound, status = D.encode_files_plan([b])
    assert kind[0] == -1 and status[0] == R.INVALID_ARG and bound[0] == 0
    long_pcm = W.wav("u8", 1, 8000, np.full(65535 * 240 * 3, 128))        # 31 250 Hz x 3.9: far past 65 535 frames
    kind, _, status = D.encode_files_plan([long_pcm])
    assert kind[0] == -1 and status[0] == R.INVALID_ARG
    ok = W.wav("u8", 1, 8000, np.full(8000 * 60, 128))                      # one minute: within the limit
    kind, _, status = D.encode_files_plan([ok])
    assert kind[0] == D.FILE_WAV and status[0] == 0


def test_extensible_chunk_past_the_end_is_bad_stream():
    """rule 8: an EXTENSIBLE fmt chunk whose 40 bytes run past the end of the file"""
    body = W.riff([W.chunk("data", bytes(60)), b"fmt " + struct.pack("<I", 40) + struct.pack("<HHIIHH", 0xFFFE, 1, 8000, 16000, 2, 16)
                   + bytes(2)])
    assert D.wav_parse(body)["status"] == R.BAD_STREAM
    assert R.parse(body)[0] == R.BAD_STREAM


@pytest.mark.parametrize("name,data", EDGE, ids=[c[0] for c in EDGE])
def test_float_edge_files_parse_and_load_as_nyquist(name, data):
    """the float-edge files: dcs_wav_parse equals the restatement, and wav_ref's values are NyquistIO::Load's floats (sha256
    over the bits, so NaN payloads and signed zeros count) wherever libnyquist reads the file as float (not EXTENSIBLE,
    rule 10)"""
    got = D.wav_parse(data)
    st, d = R.parse(data)
    assert got["status"] == st == 0, (name, got["reason"])
    for k in ("formatCode", "channels", "rate", "blockAlign", "bitDepth", "sampleFormat", "dataOffset", "dataSize", "nValues"):
        assert got[k] == d[k], (name, k)
    ref = REF[name]
    assert ref["file_sha256"] == hashlib.sha256(data).hexdigest()
    assert all(r["load"].startswith("ok") for r in ref["runs"])
    v = R.values(data, d)
    assert len(v) == ref["n_values"]
    if "_ext_" not in name:
        assert hashlib.sha256(np.asarray(v, "<f4").tobytes()).hexdigest() == ref["values_sha256"], name
    else:
        assert hashlib.sha256(np.asarray(v, "<f4").tobytes()).hexdigest() != ref["values_sha256"], name


def test_float_edge_files_hold_the_edges():
    """what the list is for, read back through the restatement: no edge is lost to a change of seed"""
    vals = {n: R.values(b, R.parse(b)[1]) for n, b in EDGE}
    raw64 = {n: np.frombuffer(b[R.parse(b)[1]["dataOffset"]:][:8 * R.parse(b)[1]["nValues"]], "<f8") for n, b in EDGE if "_f64_" in n}
    fmax, tiny = np.finfo(np.float32).max, 2.0 ** -126
    assert {R.parse(b)[1]["sampleFormat"] for _, b in EDGE} == {D.WAV_F32, D.WAV_F64}
    assert {R.parse(b)[1]["channels"] for _, b in EDGE} == {1, 2} and {R.parse(b)[1]["formatCode"] for _, b in EDGE} == {3, 0xFFFE}
    sub = vals["fe_f32_subnormal_1ch"]
    assert ((np.abs(sub) > 0) & (np.abs(sub) < tiny)).sum() > 700 and (sub.view(np.uint32) == 0x80000000).sum() > 100
    v, r = vals["fe_f64_to_subnormal_1ch"], raw64["fe_f64_to_subnormal_1ch"]
    assert (v.astype(np.float64) != r).sum() > 900 and (np.abs(v) <= tiny).all()           # every one rounds, into the range
    assert v[0] == 0 and v[1] == np.float32(2 * 2.0 ** -149) and v[2] == np.float32(2 * 2.0 ** -149)     # ties to even
    v, r = vals["fe_f64_to_zero_2ch"], raw64["fe_f64_to_zero_2ch"]
    assert (v == 0).all() and (r != 0).all() and (v.view(np.uint32) == 0x80000000).any() and (v.view(np.uint32) == 0).any()
    v, r = vals["fe_f64_to_fltmax_1ch"], raw64["fe_f64_to_fltmax_1ch"]
    assert (np.abs(v) == fmax).sum() >= 9 and not (np.abs(r) == float(fmax)).any() and np.isfinite(v).all()
    v, r = vals["fe_f64_overflow_1ch"], raw64["fe_f64_overflow_1ch"]
    assert np.isinf(v).sum() >= 9 and np.isfinite(r).all()
    assert np.isnan(vals["fe_f32_nan_1ch"]).any() and np.isposinf(vals["fe_f32_inf_2ch"]).any() and np.isneginf(vals["fe_f32_inf_2ch"]).any()
    v = vals["fe_f32_pair_overflow_2ch"]
    assert np.isfinite(v).all() and np.isinf(R.downmix(v, 2)).sum() >= 2
    one = np.float32(1)
    assert {1.0, -1.0, float(np.nextafter(one, np.float32(0)))} <= set(np.abs(vals["fe_f32_at_one_1ch"]).tolist() + vals["fe_f32_at_one_1ch"].tolist())
    assert np.abs(vals["fe_f32_above_one_1ch"]).max() == np.nextafter(one, np.float32(2))
    v, r = vals["fe_f64_rounds_to_one_1ch"], raw64["fe_f64_rounds_to_one_1ch"]
    assert np.abs(v).max() == 1.0 and np.abs(r).max() > 1.0
