"""dcs_flac_decode and dcs_encode_files on FLAC files on the MI355X: the device decode (F1 walk, F2 restore, F3 mix) against
NyquistIO::Load's floats and EncodeFile's bytes in the fixture (tests/golden/flac_golden.*, made by the reference linked with
libnyquist and its libFLAC), on the seeded files of tests/flac_cases.py; the refusals of INTEGRATION.md rules 20-25; mixed
lists; batch invariance; FLAC against the WAV file of the same integers."""
import hashlib
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import flac_cases as F
import flac_ref as R
import wav_cases as W
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_INVALID_ARG, DcsError

pytestmark = pytest.mark.gpu

CASES = F.cases()
REFUSED = F.refused_cases()
HERE = os.path.dirname(os.path.abspath(__file__))
REF = {c["name"]: c for c in json.load(open(os.path.join(HERE, "golden", "flac_golden.json")))["cases"]}
NPZ = np.load(os.path.join(HERE, "golden", "flac_golden.npz"))


def same_bits(a, b):
    return len(a) == len(b) and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def sha(x):
    return hashlib.sha256(np.asarray(x, "<f4").tobytes()).hexdigest()


def test_flac_decode_equals_nyquist_load(gpu_ctx):
    """every accepted case in one call, bit for bit: a mono file's output is Load's floats themselves (their sha256, and the
    kept bits); a stereo file's is EncodeFile's downmix of them, as flac_ref computes it from the kept bits (short cases) or
    from its own values, which test_flac_host.py ties to Load's sha256"""
    got = gpu_ctx.flac_decode([b for _, b in CASES])
    n_kept = 0
    for (name, b), y in zip(CASES, got):
        c = REF[name]
        channels = R.parse(b)[1]["channels"]
        assert len(y) == c["n_values"] // channels, name
        if channels == 1:
            assert sha(y) == c["values_sha256"], name
        if name + "/values" in NPZ:
            assert same_bits(y, R.downmix(NPZ[name + "/values"], channels)), name
            n_kept += 1
        assert same_bits(y, R.decode(b)[1]), name
    assert n_kept >= 15
    by = dict(zip([n for n, _ in CASES], got))
    assert by["fullscale_s16_31250"][0] == np.float32(-32768) / np.float32(32767)
    assert by["fullscale_s8_31250"][0] == np.float32(-128) * (np.float32(1) / np.float32(127))
    assert not by["total_larger_zero_tail"][64:].any() and by["total_larger_zero_tail"][:64].any()


@pytest.mark.parametrize("version", [0x9400, 0x9302])
def test_encode_files_equals_reference_encodefile(gpu_ctx, version):
    """bytes against the reference's own EncodeFile (which runs its converter at 31 250 Hz too: DCS_RESAMPLE_AT_UNITY)"""
    out, info = gpu_ctx.encode_files([b for _, b in CASES], version=version, at_unity=True)
    for (name, b), o, inf in zip(CASES, out, info):
        run = [r for r in REF[name]["runs"] if r["version"] == version][0]
        assert len(o) == run["bytes"] and hashlib.sha256(o).hexdigest() == run["sha256"], name
        key = "%s/%x/stream" % (name, version)
        if key in NPZ:
            assert o == NPZ[key].tobytes(), name
        d = R.parse(b)[1]
        assert inf["kind"] == D.FILE_FLAC and inf["sourceFormat"] == d["sampleFormat"], name
        assert inf["rate"] == d["rate"] and inf["channels"] == d["channels"] and inf["nValues"] == d["nValues"], name
        assert inf["enc"]["nBytes"] == run["bytes"]


def test_full_scale_negative_is_accepted(gpu_ctx):
    """rule 25: -32768 at 16 bits (-1.0000305) and -128 at 8 bits (-1.0078740) passed through at 31 250 Hz reach the encoder
    and are encoded (the reference's sanitizer screen is clean on these files)"""
    by = dict(CASES)
    out, info = gpu_ctx.encode_files([by["fullscale_s16_31250"], by["fullscale_s8_31250"]])
    assert all(len(o) > 18 for o in out) and list(info["walk"]) == [D.FILE_WALK_NONE] * 2
    assert list(info["sourceFormat"]) == [D.WAV_S16, D.WAV_S8]
    for name in ("fullscale_s16_31250", "fullscale_s8_31250"):
        assert all(r["ubsan"] == [] and r["encode"].startswith("ok") for r in REF[name]["runs"])


def _refusal(ctx, call, status, idx, *words):
    with pytest.raises(DcsError) as e:
        call()
    assert e.value.status == status
    msg = ctx.L.dcs_last_error(ctx.h).decode()
    assert msg.startswith("file %d:" % idx) and all(w in msg for w in words), msg
    return msg


@pytest.mark.parametrize("name,data,status,where,rule", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_cases(gpu_ctx, name, data, status, where, rule):
    """every clause of rules 20-25: the status, the file's index and, from the index on, the frame; a file a kernel refuses
    leaves the call with a clean error and the context usable"""
    good = dict(CASES)["types_s16_mono"]
    words = ("frame",) if where == "device" or (where == "host" and rule in (21, 23, 24) and status == ERR_BAD_STREAM) else ()
    _refusal(gpu_ctx, lambda: gpu_ctx.encode_files([good, data], at_unity=True), status, 1, *words)
    if where != "plan":
        _refusal(gpu_ctx, lambda: gpu_ctx.flac_decode([good, good, data]), status, 2, *words)
    assert same_bits(gpu_ctx.flac_decode([good])[0], R.decode(good)[1])


def test_where_the_reference_refuses_so_does_the_library():
    """what the reference did with each refused file is in the fixture: an exception from libFLAC's error callback, a crash,
    or a load (silence for 12 and 20 bits; undefined reads) -- the library refuses all of them, and nothing the reference
    throws on is among the accepted cases"""
    thrown = crashed = loaded = 0
    for name, _, _, _, _ in REFUSED:
        r = REF[name]["runs"][0]
        if r["rc"] != 0:
            crashed += 1
        elif r["load"] is None or not r["load"].startswith("ok"):
            thrown += 1
        else:
            loaded += 1
    assert thrown >= 8 and crashed >= 2 and loaded >= 3
    for name in ("r22_total_zero", "r22_total_smaller"):
        assert REF[name]["runs"][0]["rc"] != 0, name                              # the reference overruns its buffer
    for name in ("r23_crc16_flipped", "r23_crc16_flipped_last", "r23_crc8_flipped", "r23_lost_sync", "r23_reserved_subframe_type",
                 "r23_lpc_precision_1111", "r23_padding_nonzero", "r24_short_stream_trailing_junk"):
        r = REF[name]["runs"][0]
        assert r["rc"] == 0 and "FLAC" in r["load"] and not r["load"].startswith("ok"), (name, r)


def dcsa(fmt, frames, seed):
    s = D.synth_stream(fmt, frames, seed=seed)
    return D.dcsa_header(D.format_os(fmt), len(s)) + s


def test_mixed_list_keeps_input_order(gpu_ctx):
    by, wav = dict(CASES), dict(W.cases())
    files = [by["assign_s24_stereo"], wav["s16_2ch_44100"], dcsa(D.FMT_94_T0, 40, 1), by["frames_300_mono"], wav["ima_512_2ch"],
             dcsa(D.FMT_93B_T1, 30, 2), by["wasted_s16_stereo"], wav["u8_1ch_22050"], by["fullscale_s8_31250"]]
    out, info = gpu_ctx.encode_files(files)
    assert list(info["kind"]) == [D.FILE_FLAC, D.FILE_WAV, D.FILE_DCSA_COPY, D.FILE_FLAC, D.FILE_WAV, D.FILE_DCSA_REENCODE,
                                  D.FILE_FLAC, D.FILE_WAV, D.FILE_FLAC]
    for i, f in enumerate(files):                           # batch invariance: each file alone gives the same bytes
        alone, ai = gpu_ctx.encode_files([f])
        assert alone[0] == out[i] and ai[0]["kind"] == info[i]["kind"], i
    # an error in a mixed list names the file's own index
    bad = {c[0]: c[1] for c in REFUSED}["r23_sample_outside_depth"]
    _refusal(gpu_ctx, lambda: gpu_ctx.encode_files(files[:4] + [bad] + files[4:]), ERR_BAD_STREAM, 4, "frame 1", "depth")


def test_batch_of_12000_lanes_equals_single_calls(gpu_ctx):
    """the 300-frame file 40 times in one call (12 000 F1 lanes, 188 workgroups) and 40 calls of one"""
    b = dict(CASES)["frames_300_mono"]
    want = R.decode(b)[1]
    got = gpu_ctx.flac_decode([b] * 40)
    assert all(same_bits(y, want) for y in got)
    for _ in range(40):
        assert same_bits(gpu_ctx.flac_decode([b])[0], want)
    out, _ = gpu_ctx.encode_files([b] * 40)
    assert all(o == out[0] for o in out) and out[0] == gpu_ctx.encode_files([b])[0][0]


def test_flac_equals_wav_of_the_same_integers(gpu_ctx):
    """16 and 24 bits, where libnyquist converts FLAC's and WAV's integers alike: the FLAC file and the WAV file wav_cases
    builds from the integers the writer ran its recurrences to encode to the same bytes"""
    ints = F.integers()
    flacs, wavs = [], []
    for name, b in CASES:
        v, (rate, channels, bits) = ints[name]
        if bits == 8 or name.startswith("total_larger"):
            continue
        flacs.append(b)
        wavs.append(W.wav("s16" if bits == 16 else "s24", channels, rate, R.cut(v, bits)))
    assert len(flacs) >= 18
    a, ai = gpu_ctx.encode_files(flacs)
    w, wi = gpu_ctx.encode_files(wavs)
    assert a == w
    assert list(ai["nSamples"]) == list(wi["nSamples"]) and set(wi["kind"]) == {D.FILE_WAV} and set(ai["kind"]) == {D.FILE_FLAC}
    for x, y in zip(gpu_ctx.flac_decode(flacs), gpu_ctx.wav_decode(wavs)):
        assert same_bits(x, y)
