"""Which refusal wins, and what a refused call has already written, in the chain from the converter to the encoder:
dcs_encode_streams_at(_level), dcs_resample_streams_level, dcs_level_streams and dcs_encode_files(_level).  The other files
check each refusal alone; here two reasons to refuse meet in one call, and every output buffer is pre-filled with a pattern
(tests/chain_calls.py) so that a write shows.

The order the drivers keep: arguments and parameters, the rates (rsCheck), the levels, the plan of the files; then the
converter, which refuses a sample that is not finite before any gate; then per stream, in stream order, the length and then
the range of what the encoder would read (the levelled peak where a level is given).  dcs_resample_streams_level publishes
levelInfo before its capacity check and fills outOffsets on DCS_ERR_CAPACITY; dcs_level_streams checks capacity before it
runs anything; dcs_encode_streams_at_level publishes nothing on a refusal.

The inputs: a full-scale square of 1 200 samples at 44 100 Hz, which resamples to a peak of 1.2161; 3 samples at 384 000 Hz,
which resample to none; a quiet sine; the sine with one NaN.

One case differs from what one might expect of the file driver: a DCSa container of zero frames for another format family is
refused by the plan (dcsTranscodePlan, "zero frames"), which runs before the WAV group, so that file is named and not the
loud WAV file after it."""
import numpy as np
import pytest

import chain_calls as C
import dcsexplorer_amd as D
import flac_cases as FC
import wav_cases as WC
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_INVALID_ARG, LEVEL_CLIP, LEVEL_FIT, LEVEL_GAIN, Level

pytestmark = pytest.mark.gpu

F32 = np.float32
OK, ERR_CAPACITY = 0, -5
SQ = np.where((np.arange(1200) // 50) & 1, -1.0, 1.0).astype(F32)
TINY = np.full(3, 0.1, F32)
QUIET = (0.3 * np.sin(np.arange(3000) * 0.05)).astype(F32)
NAN = QUIET.copy()
NAN[100] = np.nan
FIT = Level(LEVEL_FIT)


def refused(c, status, *words):
    assert c.status == status, (c.status, c.msg)
    for w in words:
        assert w in c.msg, (w, c.msg)


def nothing_published(c):
    assert C.untouched(c.linfo) and C.untouched(c.offs, 1), (c.linfo, c.offs)


@pytest.mark.parametrize("level", [None, Level(LEVEL_GAIN, gain=1.0)], ids=["plain", "level"])
def test_encode_streams_at_first_refusal_in_stream_order(gpu_ctx, level):
    c = C.enc_at(gpu_ctx, [SQ, TINY], [44100, 384000], level=level)
    refused(c, ERR_BAD_STREAM, "stream 0", "peaks at |x| = 1.21610")
    nothing_published(c)
    c = C.enc_at(gpu_ctx, [TINY, SQ], [384000, 44100], level=level)
    refused(c, ERR_INVALID_ARG, "stream 0", "no samples")
    nothing_published(c)
    # the converter's refusal comes before every gate
    c = C.enc_at(gpu_ctx, [TINY, NAN], [384000, 48000], level=level)
    refused(c, ERR_BAD_STREAM, "stream 1", "finite")
    nothing_published(c)


def test_encode_streams_at_fit_moves_the_refusal_on(gpu_ctx):
    """with FIT stream 0 is no longer loud, and stream 1's length is what is refused"""
    c = C.enc_at(gpu_ctx, [SQ, TINY], [44100, 384000], level=FIT)
    refused(c, ERR_INVALID_ARG, "stream 1", "no samples")
    nothing_published(c)


def test_encode_streams_at_argument_order(gpu_ctx):
    bad_level = [Level(7), FIT]
    c = C.enc_at(gpu_ctx, [QUIET, QUIET], [44100, 3999], level=bad_level)
    refused(c, ERR_INVALID_ARG, "stream 1", "rate 3999")
    nothing_published(c)
    c = C.enc_at(gpu_ctx, [QUIET, QUIET], [44100, 44100], level=bad_level)
    refused(c, ERR_INVALID_ARG)
    assert c.msg.startswith("stream 0: level:"), c.msg
    nothing_published(c)
    # invalid parameters come before the rates: their message, or none (then the last call's stays)
    c = C.enc_at(gpu_ctx, [QUIET, QUIET], [44100, 3999], version=0x9301, level=bad_level, streamFormatType=1)
    refused(c, ERR_INVALID_ARG, "OS93a Type 1")
    nothing_published(c)
    c = C.enc_at(gpu_ctx, [QUIET, QUIET], [44100, 3999], level=bad_level, targetBitRate=0)
    refused(c, ERR_INVALID_ARG, "OS93a Type 1")
    assert "rate 3999" not in c.msg
    nothing_published(c)


def test_resample_streams_level_capacity(gpu_ctx):
    pcm, rates = [SQ, QUIET], [44100, 48000]
    full = C.resample(gpu_ctx, pcm, rates, level=FIT)
    assert full.status == OK and full.linfo[0]["gain"] < 1 and full.linfo[1]["gain"] == 1
    c = C.resample(gpu_ctx, pcm, rates, level=FIT, short=1)
    refused(c, ERR_CAPACITY)
    assert list(c.offs) == list(full.offs) and c.offs[2] > c.offs[1] > 0
    assert c.linfo.tobytes() == full.linfo.tobytes() and not c.linfo["nClipped"].any()
    assert C.untouched(c.out)
    # a clamp's counts are the device's: none yet where the capacity is refused
    clip = Level(LEVEL_GAIN, LEVEL_CLIP, 1.0, 1.0)
    assert C.resample(gpu_ctx, pcm, rates, level=clip).linfo[0]["nClipped"] > 0
    c = C.resample(gpu_ctx, pcm, rates, level=clip, short=1)
    refused(c, ERR_CAPACITY)
    assert list(c.offs) == list(full.offs) and not c.linfo["nClipped"].any() and c.linfo[0]["peakOut"] == 1 and C.untouched(c.out)
    c = C.resample(gpu_ctx, pcm, rates, short=1)                    # levels NULL
    refused(c, ERR_CAPACITY)
    assert list(c.offs) == list(full.offs) and C.untouched(c.out) and C.untouched(c.linfo)
    # a sample that is not finite wins over the capacity, and nothing is published
    c = C.resample(gpu_ctx, [QUIET, NAN], [48000, 48000], level=FIT, short=1)
    refused(c, ERR_BAD_STREAM, "stream 1", "finite")
    assert C.untouched(c.linfo) and C.untouched(c.out)
    for level in (None, FIT):
        c = C.resample(gpu_ctx, [], [], level=level)
        assert c.status == OK and c.offs[0] == 0


def test_level_streams_capacity_wins(gpu_ctx):
    c = C.level_streams(gpu_ctx, [QUIET, NAN], FIT, short=1)
    refused(c, ERR_CAPACITY)
    assert list(c.offs) == [0, 3000, 6000] and C.untouched(c.linfo) and C.untouched(c.out)
    c = C.level_streams(gpu_ctx, [QUIET, NAN], FIT)
    refused(c, ERR_BAD_STREAM, "stream 1", "a sample is not finite")
    assert list(c.offs) == [0, 3000, 6000] and C.untouched(c.linfo)


def dcsa(fmt, frames, seed):
    s = D.synth_stream(fmt, frames, seed=seed)
    return D.dcsa_header(D.format_os(fmt), len(s)) + s


def test_encode_files_order(gpu_ctx):
    wav = dict(WC.cases())
    loud, quiet, refused_by_plan = wav["fullscale_s16_31250"], wav["s16_1ch_22050"], wav["err_mulaw"]
    c = C.encode_files(gpu_ctx, [loud], at_unity=True)
    refused(c, ERR_BAD_STREAM, "file 0", "peaks at")
    # the plan's refusal of file 1 comes before file 0's peak
    c = C.encode_files(gpu_ctx, [loud, refused_by_plan], at_unity=True)
    refused(c, ERR_INVALID_ARG, "file 1", "format code")
    assert C.untouched(c.offs, 1) and C.untouched(c.info) and C.untouched(c.out)
    # a container of zero frames for another family is refused in the plan as well, ahead of the WAV group
    empty = D.dcsa_header(D.format_os(D.FMT_94_T0), 4) + bytes(4)
    c = C.encode_files(gpu_ctx, [empty, loud], version=0x9302, at_unity=True)
    refused(c, ERR_BAD_STREAM, "file 0", "zero frames")
    assert C.untouched(c.offs, 1) and C.untouched(c.info)
    # past the plan the WAV group runs first: its file 1 is named although the container is file 0
    c = C.encode_files(gpu_ctx, [dcsa(D.FMT_94_T0, 10, 3), loud], version=0x9302, at_unity=True)
    refused(c, ERR_BAD_STREAM, "file 1", "peaks at")
    assert C.untouched(c.offs, 1) and C.untouched(c.info)
    # the levels are checked before the files are read
    c = C.encode_files(gpu_ctx, [b"junk" * 20, quiet], level=[FIT, Level(LEVEL_GAIN, gain=-1.0)])
    refused(c, ERR_INVALID_ARG)
    assert c.msg.startswith("file 1: level:"), c.msg
    assert C.untouched(c.linfo) and C.untouched(c.offs, 1)


def test_encode_files_capacity_and_empty_list(gpu_ctx):
    wav, flac = dict(WC.cases()), dict(FC.cases())
    files = [wav["s16_1ch_22050"], dcsa(D.FMT_94_T0, 10, 3), flac["fullscale_s16_31250"], wav["fullscale_s16_31250"]]
    full = C.encode_files(gpu_ctx, files, level=FIT)
    assert full.status == OK and full.linfo[3]["gain"] < 1
    c = C.encode_files(gpu_ctx, files, level=FIT, short=1)
    refused(c, ERR_CAPACITY)
    assert list(c.offs) == list(full.offs) and c.info.tobytes() == full.info.tobytes() and c.linfo.tobytes() == full.linfo.tobytes()
    assert tuple(c.linfo[1]) == (0.0, 1.0, 0.0, 0, 0) and C.untouched(c.out)
    for level in (None, FIT):
        c = C.encode_files(gpu_ctx, [], level=level)
        assert c.status == OK and c.offs[0] == 0
