"""dcs_encode_files and dcs_wav_decode on the MI355X.  The device unpack (W0, W1) against the numpy restatement of
libnyquist's reader (tests/wav_ref.py), exhaustively for int16 and u8 and over 24- and 32-bit sweeps with the extremes;
encode_files against its composition from pieces the earlier fixtures pin (wav_ref, then encode_streams_at, and
transcode_dcsa for DCSa files); batch invariance; the host and device routes of the resampler's walk giving the same bytes on
a 180-second file; errors naming the file; the capacity protocol."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import resample_ref as RS
import wav_cases as W
import wav_ref as R
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_CAPACITY, ERR_INVALID_ARG, DcsError, _files_blob, _ptr, transcode_params

pytestmark = pytest.mark.gpu

CASES = W.cases()
EDGE = W.float_edge_cases()
HERE = os.path.dirname(os.path.abspath(__file__))
REF = json.load(open(os.path.join(HERE, "golden", "encode_file_golden.json")))
REF_RUN = {(c["name"], r["version"]): r for c in REF["cases"] for r in c["runs"]}
GOOD = [(n, b) for n, b in CASES if R.parse(b)[0] == 0]


def same_bits(a, b):
    return len(a) == len(b) and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def composed(ctx, data, version=0x9400):
    """EncodeFile's WAV path from pieces: the restated reader and downmix, then encode_streams_at at the file's rate"""
    st, mono, d = R.decode(data)
    assert st == 0
    out, info = ctx.encode_streams_at([mono], d["rate"], version)
    return out[0], info[0]


def test_wav_decode_every_case(gpu_ctx):
    got = gpu_ctx.wav_decode([b for _, b in GOOD])
    for (name, b), y in zip(GOOD, got):
        assert same_bits(y, R.decode(b)[1]), name


def test_wav_decode_exhaustive(gpu_ctx):
    i16 = np.arange(-32768, 32768, dtype=np.int64)
    u8 = np.arange(256, dtype=np.int64)
    i24 = np.concatenate([np.arange(-(1 << 23), -(1 << 23) + 4096), np.arange(-70000, 70000), np.arange((1 << 23) - 4096, 1 << 23),
                          np.random.default_rng(24).integers(-(1 << 23), 1 << 23, 100000)])
    i32 = np.concatenate([np.array([-(1 << 31), -(1 << 31) + 1, -1, 0, 1, (1 << 31) - 1]),
                          np.random.default_rng(32).integers(-(1 << 31), 1 << 31, 200000), np.arange(-(1 << 31), -(1 << 31) + 300000, 7)])
    files = [W.wav("s16", 1, 8000, i16), W.wav("u8", 1, 8000, u8), W.wav("s24", 1, 8000, i24), W.wav("s32", 1, 8000, i32),
             W.wav("s16", 2, 8000, i16)]
    got = gpu_ctx.wav_decode(files)
    for b, y in zip(files, got):
        assert same_bits(y, R.decode(b)[1])
    assert got[0][0] == np.float32(-32768) / np.float32(32767) and got[0][-1] == 1.0
    assert got[1][0] == (np.float32(0) - np.float32(128)) * (np.float32(1) / np.float32(127))


def test_wav_decode_adpcm_blocks(gpu_ctx):
    ima = [(n, b) for n, b in GOOD if n.startswith("ima_")] + [("ima_wrap", W.ima_wrap_wav())]
    assert len(ima) >= 7
    for (name, b), y in zip(ima, gpu_ctx.wav_decode([b for _, b in ima])):
        st, mono, d = R.decode(b)
        assert same_bits(y, mono), name
        assert d["nBlocks"] >= 1


@pytest.mark.parametrize("version", [0x9400, 0x9302])
def test_encode_files_every_case(gpu_ctx, version):
    enc = [(n, b) for n, b in GOOD if not n.startswith(("fullscale_", "enc_err_"))]
    out, info = gpu_ctx.encode_files([b for _, b in enc], version=version)
    for (name, b), o, inf in zip(enc, out, info):
        want, wi = composed(gpu_ctx, b, version)
        assert o == want, name
        st, d = R.parse(b)
        assert inf["kind"] == D.FILE_WAV and inf["rate"] == d["rate"] and inf["channels"] == d["channels"], name
        assert inf["nValues"] == d["nValues"] and inf["sourceFormat"] == d["formatCode"]
        assert tuple(inf["enc"]) == tuple(wi)
        assert inf["walk"] == (D.FILE_WALK_NONE if d["rate"] == 31250 else D.FILE_WALK_DEVICE)


def test_full_scale_negative_is_accepted(gpu_ctx):
    """rule 12: int16 -32768 (-1.0000305) and u8 0 (-1.0078740) passed through at 31 250 Hz are encoded, as the reference
    encodes them (its sanitizer screen is clean on these cases); beyond the format's own full scale is still refused, and so
    is the filter's overshoot past it"""
    by = dict(CASES)
    out, info = gpu_ctx.encode_files([by["fullscale_s16_31250"], by["fullscale_u8_31250"]])
    assert all(len(o) > 0 for o in out) and list(info["walk"]) == [D.FILE_WALK_NONE] * 2
    # through the converter at unity the sinc filter overshoots to 1.044, beyond either bound: refused, naming the file
    with pytest.raises(DcsError) as e:
        gpu_ctx.encode_files([by["s16_1ch_22050"], by["fullscale_s16_31250"]], at_unity=True)
    assert e.value.status == ERR_BAD_STREAM
    assert gpu_ctx.L.dcs_last_error(gpu_ctx.h).decode().startswith("file 1:")
    with pytest.raises(DcsError) as e:                      # float input keeps the bound of 1
        gpu_ctx.encode_files([by["s16_1ch_22050"], W.wav("f32", 1, 31250, np.full(500, -1.0001))])
    assert e.value.status == ERR_BAD_STREAM
    assert gpu_ctx.L.dcs_last_error(gpu_ctx.h).decode().startswith("file 1:")
    with pytest.raises(DcsError):                           # the encoder entry points keep theirs
        gpu_ctx.encode_streams_at([np.full(500, np.float32(-32768) / np.float32(32767))], 31250)


# Where the library departs from what the reference does with the file (INTEGRATION.md rules 8-12 and 19, and the resampler's
# rate range): it refuses the file, or reads it differently (rule 10), so the reference's bytes are not the contract there
DEPARTS = {"ext_float_f32": 10, "ext_float_f64": 10, "err_mulaw": 9, "err_bits12": 9, "err_int64": 9, "err_ext_other": 10,
           "err_3ch": 9, "err_data_past_end": 8, "err_blockalign0": 8, "err_ima_no_fact": 11, "err_ima_step89": 11,
           "err_ima_overflow": 11, "enc_err_rate_low": 0, "fullscale_s16_31250": 12, "fullscale_u8_31250": 12,
           # float files (tests/wav_cases.py float_edge_cases): EXTENSIBLE float is read as float (rule 10); a value or a pair's
           # mean that is not finite, and a float value above 1 that reaches the encoder, are refused (rule 19), where the
           # reference encodes them -- the first kind through casts its sanitizer build reports; a full-scale DC level
           # overshoots in the converter (rule 12)
           "fe_ext_f32_subnormal_2ch": 10, "fe_ext_f64_to_subnormal_1ch": 10, "fe_ext_f32_inf_1ch": 10,
           "fe_f64_overflow_1ch": 19, "fe_f32_nan_1ch": 19, "fe_f32_inf_2ch": 19, "fe_f64_inf_1ch": 19,
           "fe_f32_pair_overflow_2ch": 19, "fe_f64_to_fltmax_1ch": 19, "fe_f32_fltmax_1ch": 19,
           "fe_f32_dc_above_one_1ch": 19, "fe_f64_dc_above_one_2ch": 19, "fe_f32_dc_one_1ch": 12}


@pytest.mark.parametrize("version", [0x9400, 0x9302])
def test_encode_files_equals_reference_encodefile(gpu_ctx, version):
    """bytes and refusals against the reference's own EncodeFile linked with libnyquist (tests/golden/encode_file_golden.*)"""
    by = dict(CASES + EDGE)
    acc, n_ref_refused = [], 0
    for c in REF["cases"]:
        name = c["name"]
        if name.startswith("long_"):
            continue
        run = REF_RUN[name, version]
        ours = R.parse(by[name])[0]
        if name in DEPARTS:
            assert ours != 0 or DEPARTS[name] in (0, 10, 12, 19), name
            continue
        if run["encode"] is None or not run["encode"].startswith("ok"):
            assert ours != 0, name                          # the reference refuses it: so does the library
            with pytest.raises(DcsError):
                gpu_ctx.encode_files([by[name]], version=version, at_unity=True)
            n_ref_refused += 1
            continue
        assert ours == 0 and run["ubsan"] in ([], ["shift"]), name
        acc.append(name)
    # EncodeFile runs the converter at 31 250 Hz too: DCS_RESAMPLE_AT_UNITY
    out, info = gpu_ctx.encode_files([by[n] for n in acc], version=version, at_unity=True)
    for name, o, inf in zip(acc, out, info):
        run = REF_RUN[name, version]
        assert len(o) == run["bytes"] and hashlib.sha256(o).hexdigest() == run["sha256"], name
        assert inf["enc"]["nBytes"] == run["bytes"]
    assert len(acc) >= 70 and n_ref_refused >= 5


def test_wav_decode_equals_nyquist_load(gpu_ctx):
    """the values before the downmix are NyquistIO::Load's: every case's float sha256 through wav_ref, and the mono cases
    (whose output is Load's floats themselves) through dcs_wav_decode; the float-edge cases are among them"""
    by = dict(CASES + EDGE)
    for c in REF["cases"]:
        name = c["name"]
        if name in DEPARTS or name.startswith("long_") or "values_sha256" not in c or R.parse(by[name])[0] != 0:
            continue
        st, d = R.parse(by[name])
        v = R.values(by[name], d)
        assert hashlib.sha256(np.asarray(v, "<f4").tobytes()).hexdigest() == c["values_sha256"], name
        if d["channels"] == 1:
            y = gpu_ctx.wav_decode([by[name]])[0]
            assert hashlib.sha256(np.asarray(y, "<f4").tobytes()).hexdigest() == c["values_sha256"], name


def test_float_edges_decode_to_the_restated_bits(gpu_ctx):
    """subnormals, -0.0, f64 values rounding into the subnormal range, to +-0, to FLT_MAX and past it, NaN and +-inf: the
    device unpack gives wav_ref's bits (a NaN only where it is copied, so its payload is the file's), alone and in a batch"""
    got = gpu_ctx.wav_decode([b for _, b in EDGE])
    for (name, b), y in zip(EDGE, got):
        want = R.decode(b)[1]
        assert same_bits(y, want), name
        assert same_bits(gpu_ctx.wav_decode([b])[0], want), name
    flat = np.concatenate(got)
    a = np.abs(flat)
    # (-0.0: the 500 pairs of the all -0.0 file and every seventh value of the mono subnormal file, 143, at the least)
    assert ((a > 0) & (a < 2.0 ** -126)).sum() > 3000 and (flat.view(np.uint32) == 0x80000000).sum() >= 643
    assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any() and (a == np.finfo(np.float32).max).any()


def test_more_than_65535_files_in_one_decode(gpu_ctx):
    """70 001 small f32 files drawn from 56 distinct ones (5 to 60 values of the float-edge kinds, mono and stereo):
    wavUnpackKernel's blockIdx.y loop takes a second pass, and every file still decodes to its own bits"""
    rng = np.random.default_rng(0x70001)
    src = np.concatenate([R.values(b, R.parse(b)[1]) for n, b in EDGE if "_f32_" in n and "nan" not in n and "_ext_" not in n])
    pool = []
    for k in range(56):
        n, ch = int(rng.integers(5, 61)), 1 + k % 2
        n += n % ch
        at = int(rng.integers(0, len(src) - n))
        pool.append(W.wav("f32", ch, (8000, 22050, 44100, 48000)[k % 4], src[at:at + n]))
    want = [R.decode(b)[1] for b in pool]
    assert all(len(b) >= 64 for b in pool) and any(np.isinf(w).any() for w in want) and any((np.abs(w) < 2.0 ** -126).all() for w in want)
    idx = rng.integers(0, len(pool), 70001)
    idx[:len(pool)] = idx[-len(pool):] = np.arange(len(pool))
    got = gpu_ctx.wav_decode([pool[i] for i in idx])
    assert len(got) == 70001 > 65535
    bad = [k for k, (i, y) in enumerate(zip(idx, got)) if not same_bits(y, want[i])]
    assert not bad, (len(bad), bad[:5])


def _refused(ctx, good, data, *words, **kw):
    with pytest.raises(DcsError) as e:
        ctx.encode_files([good, data], **kw)
    assert e.value.status == ERR_BAD_STREAM
    msg = ctx.L.dcs_last_error(ctx.h).decode()
    assert msg.startswith("file 1:") and all(w in msg for w in words), msg
    return msg


def test_float_edges_refusals_name_the_file(gpu_ctx):
    """rule 19: a float file with a value, or a pair's mean, that is not finite is refused as such, and one whose signal
    passes 1 where the encoder reads it is refused with its peak -- decided by wav_ref's floats and the restated converter,
    not by the kernel's.  Every departure listed for these files is one of the two; every other file encodes."""
    good = dict(CASES)["s16_1ch_22050"]
    c, inc = D.resample_filter_default()
    n_finite = n_peak = n_ok = 0
    for name, b in EDGE:
        st, mono, d = R.decode(b)
        assert st == 0, name
        if not np.isfinite(mono).all():
            _refused(gpu_ctx, good, b, "finite", at_unity=True)
            _refused(gpu_ctx, good, b, "finite")
            assert DEPARTS.get(name) in (19, 10), name
            n_finite += 1
            continue
        with np.errstate(over="ignore"):
            peak = float(np.abs(RS.convert(mono, d["rate"], c, inc, RS.AT_UNITY)).max())
        if peak > 1.0:
            _refused(gpu_ctx, good, b, "peaks at", at_unity=True)
            assert DEPARTS.get(name) in (19, 12), name
            n_peak += 1
        else:
            out, _ = gpu_ctx.encode_files([good, b], at_unity=True)
            assert len(out[1]) >= 18 and (name not in DEPARTS or DEPARTS[name] == 10), name
            n_ok += 1
    assert n_finite >= 6 and n_peak >= 5 and n_ok >= 14
    by = dict(EDGE)
    # at 31 250 Hz without the converter the encoder reads the file's own values: +-1 and 1 - 2^-24 pass, 1 + 2^-23 does not
    out, info = gpu_ctx.encode_files([by["fe_f32_at_one_1ch"], by["fe_f32_dc_one_1ch"]])
    assert all(len(o) > 18 for o in out) and list(info["walk"]) == [D.FILE_WALK_NONE] * 2
    for name in ("fe_f32_above_one_1ch", "fe_f32_dc_above_one_1ch", "fe_f64_dc_above_one_2ch"):
        msg = _refused(gpu_ctx, good, by[name], "peaks at")
        assert "1.00000012" in msg, msg


def dcsa(fmt, frames, seed):
    s = D.synth_stream(fmt, frames, seed=seed)
    return D.dcsa_header(D.format_os(fmt), len(s)) + s


def test_mixed_list_equals_composition(gpu_ctx):
    by = dict(CASES)
    files = [by["s16_2ch_44100"], dcsa(D.FMT_94_T0, 40, 1), by["ima_512_2ch"], dcsa(D.FMT_93B_T1, 30, 2), by["f32_1ch_48000"]]
    out, info = gpu_ctx.encode_files(files)
    kinds = [D.FILE_WAV, D.FILE_DCSA_COPY, D.FILE_WAV, D.FILE_DCSA_REENCODE, D.FILE_WAV]
    assert list(info["kind"]) == kinds
    for i in (0, 2, 4):
        assert out[i] == composed(gpu_ctx, files[i])[0]
    t_out, t_info = gpu_ctx.transcode_dcsa([files[1], files[3]])
    assert out[1] == t_out[0][36:] and out[3] == t_out[1][36:]
    for k, i in enumerate((1, 3)):
        assert info[i]["srcFrames"] == t_info[k]["srcFrames"] and tuple(info[i]["enc"]) == tuple(t_info[k]["enc"])
    # batch invariance: each file alone gives the same bytes
    for i, f in enumerate(files):
        assert gpu_ctx.encode_files([f])[0][0] == out[i]


def test_long_file_host_and_device_walk(gpu_ctx):
    """the 180 s file alone walks on the host; inside a batch of five equal files each walks on a device lane; same bytes"""
    b = W.long_wav()
    out1, info1 = gpu_ctx.encode_files([b])
    assert info1[0]["walk"] == D.FILE_WALK_HOST
    assert hashlib.sha256(out1[0]).hexdigest() == REF_RUN["long_180s_s16_stereo_44100", 0x9400]["sha256"]
    out5, info5 = gpu_ctx.encode_files([b] * 5)
    assert list(info5["walk"]) == [D.FILE_WALK_DEVICE] * 5
    assert all(o == out1[0] for o in out5)
    assert info1[0]["nSamples"] == D.resample_count(180 * 44100 * 2, 44100, 2)
    assert info1[0]["enc"]["nFrames"] == -(-int(info1[0]["nSamples"]) // 240)


def test_errors_name_the_file(gpu_ctx):
    by = dict(CASES)
    L, h = gpu_ctx.L, gpu_ctx.h
    for files, status, idx in (([by["s16_1ch_8000"], b"xyz" * 30], ERR_INVALID_ARG, 1),
                               ([by["s16_1ch_8000"], by["u8_1ch_8000"], by["err_ima_step89"]], ERR_BAD_STREAM, 2),
                               ([by["enc_err_rate_low"]], ERR_INVALID_ARG, 0),
                               ([dcsa(D.FMT_94_T0, 10, 3), by["err_data_past_end"]], ERR_BAD_STREAM, 1)):
        with pytest.raises(DcsError) as e:
            gpu_ctx.encode_files(files)
        assert e.value.status == status
        msg = L.dcs_last_error(h).decode()
        assert msg.startswith("file %d:" % idx), msg


def test_capacity_protocol(gpu_ctx):
    by = dict(CASES)
    files = [by["s16_2ch_44100"], dcsa(D.FMT_94_T0, 20, 4), by["u8_1ch_22050"]]
    want, _ = gpu_ctx.encode_files(files)
    blob, offs = _files_blob(files)
    p = transcode_params(0x9400, None)
    out = np.zeros(16, np.uint8)
    out_offs = np.zeros(4, np.uint64)
    info = np.zeros(3, D.ENCODE_FILE_INFO_DTYPE)
    st = gpu_ctx.L.dcs_encode_files(gpu_ctx.h, _ptr(blob), _ptr(offs), 3, ctypes.byref(p), None, 0, _ptr(out), 16, _ptr(out_offs),
                                    _ptr(info))
    assert st == ERR_CAPACITY
    assert list(np.diff(out_offs)) == [len(w) for w in want]
    out = np.zeros(int(out_offs[-1]), np.uint8)
    st = gpu_ctx.L.dcs_encode_files(gpu_ctx.h, _ptr(blob), _ptr(offs), 3, ctypes.byref(p), None, 0, _ptr(out), out.size,
                                    _ptr(out_offs), _ptr(info))
    assert st == 0 and out.tobytes() == b"".join(want)
