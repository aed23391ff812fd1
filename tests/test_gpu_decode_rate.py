"""Decoding at an output rate on the GPU: dcs_resample_out_streams and dcs_decode_streams_at against the numpy restatement
(tests/decode_rate_ref.py, pinned to libsamplerate by tests/test_decode_rate_host.py) and its goldens, sample for sample.
Shapes are the smallest at which the converter can go wrong: lengths around the 16-sample call and the FLAC block, a stream
long enough for several blocks of the convolve kernel, more streams than blockIdx.y can number, both table variants (the
`big` table is past the LDS variant's 16 384 coefficients), and the long table for which the flush cap binds."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import decode_rate_ref as Q
import romkit

import dcsexplorer_amd as D
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_CAPACITY, ERR_INVALID_ARG, RATE_INFO_DTYPE, DcsError, _ptr
from oracle.rsref import big_table

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = np.load(os.path.join(HERE, "golden", "resample_filters.npz"))
GOLD = json.load(open(os.path.join(HERE, "golden", "decode_rate_golden.json")))
GOLD_ARR = np.load(os.path.join(HERE, "golden", "decode_rate_golden.npz"))
# one call's mix: every length of the issue's list, every signal; square:4080 is the clip case
MIX = ("noise:1:11", "dc+:15:0", "dc-:16:0", "impulse:17:0", "silence:240:0", "square:4080:0", "noise:4097:12", "noise:20000:13",
       "noise:240:14", "dc+:4080:0")


@functools.lru_cache(maxsize=None)
def table(name):
    if name == "long":
        return GOLD_ARR["long/coeffs"], int(GOLD_ARR["long/increment"])
    if name == "big":
        return big_table(*table("default"))
    return FILTERS[name + "/coeffs"], int(FILTERS[name + "/increment"])


def same_info(info, want, what):
    assert int(info["nIn"]) == want["nIn"] and int(info["nOut"]) == want["nOut"], what
    assert int(info["nClipped"]) == want["nClipped"], what
    assert info["peak"].view(np.uint32) == want["peak"].view(np.uint32), what
    assert int(info["reserved"]) == 0, what


def check_mix(ctx, tab, rate, at_unity):
    c, inc = table(tab)
    pcm = [Q.case_pcm(k) for k in MIX]
    out, info = ctx.resample_out_streams(pcm, rate, None if tab == "default" else (c, inc), at_unity=at_unity)
    assert len(out) == len(MIX) and info.dtype == RATE_INFO_DTYPE
    for k, key in enumerate(MIX):
        want, want_info = Q.convert(pcm[k], rate, c, inc, Q.AT_UNITY if at_unity else 0)
        print("%s %d %s: %d -> %d samples, %d clipped, peak %.6f" % (tab, rate, key, len(pcm[k]), len(want), want_info["nClipped"],
                                                                    want_info["peak"]))
        assert np.array_equal(out[k], want), (tab, rate, key, len(out[k]), len(want))
        same_info(info[k], want_info, (tab, rate, key))
    return info


@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000, 65535])
def test_resample_out_streams_default_table(gpu_ctx, rate):
    info = check_mix(gpu_ctx, "default", rate, False)
    if rate in (44100, 48000):
        assert int(info[MIX.index("square:4080:0")]["nClipped"]) > 0


def test_resample_out_streams_equals_the_goldens(gpu_ctx):
    """the library against libsamplerate's recorded output itself, the default table's short cases at every rate"""
    cases = [k for k in GOLD["cases"] if k["table"] == "default" and int(k["signal"].split(":")[1]) <= 4097]
    for rate in sorted({k["rate"] for k in cases}):
        mine = [k for k in cases if k["rate"] == rate]
        out, info = gpu_ctx.resample_out_streams([Q.case_pcm(k["signal"]) for k in mine], rate, at_unity=True)
        for y, i, k in zip(out, info, mine):
            assert len(y) == k["count"] and hashlib.sha256(y.tobytes()).hexdigest() == k["sha256"], k["name"]
            assert int(i["nClipped"]) == k["clippedHigh"] + k["clippedLow"], k["name"]
            assert int(i["peak"].view(np.uint32)) == k["peakBits"], k["name"]


def test_resample_out_streams_at_the_dcs_rate(gpu_ctx):
    """31 250 Hz: without the flag the samples come back untouched; with it the converter runs at ratio 1"""
    pcm = [Q.case_pcm(k) for k in MIX]
    out, info = gpu_ctx.resample_out_streams(pcm, 31250)
    for k in range(len(MIX)):
        assert np.array_equal(out[k], pcm[k])
        same_info(info[k], Q.convert(pcm[k], 31250, *table("default"))[1], MIX[k])
    check_mix(gpu_ctx, "default", 31250, True)


@pytest.mark.parametrize("tab,rate", [("big", 8000), ("big", 48000), ("long", 44100), ("long", 48000), ("long", 65535), ("long", 4000)])
def test_resample_out_streams_other_tables(gpu_ctx, tab, rate):
    assert (len(table("big")[0]) > 16384) and len(table("long")[0]) <= 16384
    check_mix(gpu_ctx, tab, rate, False)
    if tab == "long" and rate >= 44100:
        # the flush cap binds: the walk without it makes more outputs
        c, inc = table("long")
        assert Q._walk(4097, len(c), inc, rate, 1 << 30)[0].size > Q.count(4097, rate, len(c), inc)


def test_more_streams_than_block_rows(gpu_ctx):
    """70 001 streams of 16 samples at 48 kHz: every kernel's blockIdx.y loop takes a second pass"""
    n = 70001
    pool = [Q.signal("noise", 16, 100 + j) for j in range(7)] + [Q.signal("dc+", 16), Q.signal("square", 16)]
    want = [Q.convert(p, 48000, *table("default")) for p in pool]
    index = (np.arange(n) * 5 + (np.arange(n) // 9) % 3) % len(pool)
    out, info = gpu_ctx.resample_out_streams([pool[j] for j in index], 48000)
    assert len(out) == n
    h_got, h_want = hashlib.sha256(), hashlib.sha256()
    for k, j in enumerate(index):
        h_got.update(out[k].tobytes())
        h_want.update(want[j][0].tobytes())
    assert h_got.hexdigest() == h_want.hexdigest()
    assert np.array_equal(info["nOut"], np.array([want[j][1]["nOut"] for j in index], np.uint64))
    assert np.array_equal(info["nIn"], np.full(n, 16, np.uint64))
    assert np.array_equal(info["nClipped"], np.array([want[j][1]["nClipped"] for j in index], np.uint64))
    assert np.array_equal(info["peak"].view(np.uint32), np.array([want[j][1]["peak"].view(np.uint32) for j in index], np.uint32))
    for k in (0, 65534, 65535, 65536, n - 1):
        assert np.array_equal(out[k], want[index[k]][0]), k


@functools.lru_cache(maxsize=None)
def synthetic_streams():
    """seeded synthetic streams of 1, 2, 3, 17 and 300 frames over all six unpack layouts"""
    return [(D.format_os(f), D.synth_stream(f, n, seed=0xD0 + 16 * f + i, nbands=18 if f == D.FMT_93A_T1 else 16), 255, 0x64)
            for f in range(6) for i, n in enumerate((1, 2, 3, 17, 300))]


_DECODED = {}


def decoded(ctx, extra_frames):
    """decode_streams' PCM of the list, computed once per extra_frames and left unchanged"""
    if extra_frames not in _DECODED:
        _DECODED[extra_frames] = ctx.decode_streams(list(synthetic_streams()), extra_frames=extra_frames)
    return _DECODED[extra_frames]


@pytest.mark.parametrize("extra_frames", [0, 2])
@pytest.mark.parametrize("rate", [44100, 48000])
def test_decode_streams_at_equals_decode_then_restatement(gpu_ctx, rate, extra_frames):
    streams = list(synthetic_streams())
    pcm, err, first = decoded(gpu_ctx, extra_frames)
    out, info, got_err, got_first = gpu_ctx.decode_streams_at(streams, rate, extra_frames=extra_frames)
    assert np.array_equal(got_err, err) and np.array_equal(got_first, first)
    assert len(out) == len(streams)
    for k in range(len(streams)):
        want, want_info = Q.convert(pcm[first[k]:first[k + 1]].ravel(), rate, *table("default"))
        assert np.array_equal(out[k], want), (k, len(out[k]), len(want))
        same_info(info[k], want_info, k)
    if rate == 48000 and extra_frames == 0:
        assert {len(o) for o in out} >= {6266}             # 17 frames: a full FLAC block and 2 170 samples more


def test_decode_streams_at_as_a_sequence(gpu_ctx):
    """DCS_OUT_SEQUENCE decodes as decode_stream_sequence does: one decoder object for the list"""
    streams = [s for s in synthetic_streams() if s[0] == D.OS94][:4]
    levels = [0x64, 0x50, 0x64, 0x40]
    pcm, err, first = gpu_ctx.decode_stream_sequence(D.OS94, 255, [s[1] for s in streams], levels, extra_frames=2)
    seq = [(D.OS94, s[1], 255, lv) for s, lv in zip(streams, levels)]
    out, info, got_err, got_first = gpu_ctx.decode_streams_at(seq, 44100, extra_frames=2, sequence=True)
    assert np.array_equal(got_err, err) and np.array_equal(got_first, first)
    for k in range(len(seq)):
        want, want_info = Q.convert(pcm[first[k]:first[k + 1]].ravel(), 44100, *table("default"))
        assert np.array_equal(out[k], want), k
        same_info(info[k], want_info, k)
    with pytest.raises(DcsError) as e:                      # the sequence's own rule: at least two taper frames
        gpu_ctx.decode_streams_at(seq, 44100, extra_frames=1, sequence=True)
    assert e.value.status == ERR_INVALID_ARG


def test_decode_streams_at_capacity_protocol(gpu_ctx):
    """too small: DCS_ERR_CAPACITY, offsets and info valid, the buffer untouched; then the same call with that capacity"""
    streams = list(synthetic_streams())[:5]
    good, good_info, err, first = gpu_ctx.decode_streams_at(streams, 48000, extra_frames=2)
    need = sum(len(g) for g in good)
    refs, keep = D.api._stream_refs(streams)
    L = gpu_ctx.L
    for cap, status in ((need - 1, ERR_CAPACITY), (0, ERR_CAPACITY), (need, 0)):
        out = np.full(need + 8, 0x5A5A, np.int16)
        out_offs = np.zeros(len(streams) + 1, np.uint64)
        info = np.zeros(len(streams), RATE_INFO_DTYPE)
        got_err = np.zeros(len(err), np.uint32)
        st = L.dcs_decode_streams_at(gpu_ctx.h, refs, len(streams), 2, 48000, None, 0, _ptr(out), cap, _ptr(out_offs), _ptr(info),
                                     _ptr(got_err))
        assert st == status, cap
        assert list(out_offs) == [0] + list(np.cumsum([len(g) for g in good])), cap
        assert np.array_equal(info, good_info) and np.array_equal(got_err, err), cap
        if status == 0:
            assert np.array_equal(out[:need], np.concatenate(good)) and (out[need:] == 0x5A5A).all()
        else:
            assert (out == 0x5A5A).all()
    out_offs[:] = 0
    assert L.dcs_decode_streams_at(gpu_ctx.h, refs, len(streams), 2, 48000, None, 0, None, 0, _ptr(out_offs), None, None) == ERR_CAPACITY
    assert int(out_offs[-1]) == need
    del keep


def test_refused_calls_name_their_reason_and_leave_the_context_usable(gpu_ctx):
    good = Q.case_pcm("noise:240:14")
    want = Q.convert(good, 48000, *table("default"))[0]
    bad_table = (np.zeros(2, np.float32), 1)
    for pcm, rate, filt, word in (([good], 3999, None, "rate"), ([good], 65536, None, "rate"), ([good, np.zeros(0, np.int16)], 48000, None, "stream 1"),
                                  ([good], 48000, bad_table, "filter")):
        with pytest.raises(DcsError) as e:
            gpu_ctx.resample_out_streams(pcm, rate, filt)
        assert e.value.status == ERR_INVALID_ARG and word in str(e.value), str(e.value)
        assert np.array_equal(gpu_ctx.resample_out_streams([good], 48000)[0][0], want)
    streams = list(synthetic_streams())[:2]
    refs, keep = D.api._stream_refs(streams)
    out_offs = np.zeros(3, np.uint64)
    for rate, flags in ((48000, 4), (48000, 8 | 2), (70000, 0), (1000, 0)):
        st = gpu_ctx.L.dcs_decode_streams_at(gpu_ctx.h, refs, 2, 2, rate, None, flags, None, 0, _ptr(out_offs), None, None)
        assert st == ERR_INVALID_ARG, (rate, flags)
    with pytest.raises(DcsError) as e:
        gpu_ctx.decode_streams_at(streams, 70000)
    assert "rate" in str(e.value)
    # the decode's own refusals are named too: the sequence's rules, an empty list, unknown flags
    seq = [s for s in synthetic_streams() if s[0] == D.OS94][:2]
    for lst, extra, word in ((seq, 1, "2 extra frames"), ([seq[0], (seq[1][0], seq[1][1], 200, 0x64)], 2, "stream 1"), ([], 2, "no streams")):
        with pytest.raises(DcsError) as e:
            gpu_ctx.decode_streams_at(lst, 48000, extra_frames=extra, sequence=True)
        assert e.value.status == ERR_INVALID_ARG and "dcs_decode_streams_at" in str(e.value) and word in str(e.value), str(e.value)
    st = gpu_ctx.L.dcs_decode_streams_at(gpu_ctx.h, refs, 2, 2, 48000, None, 4, None, 0, _ptr(out_offs), None, None)
    assert st == ERR_INVALID_ARG and b"unknown flags" in gpu_ctx.L.dcs_last_error(gpu_ctx.h)
    # a stream of no frames decodes to no samples: refused before the decode is queued, by the index pass or as "empty"
    none = (streams[0][0], bytes(2) + bytes(streams[0][1][2:]), 255, 0x64)
    with pytest.raises(DcsError) as e:
        gpu_ctx.decode_streams_at([streams[1], none], 48000)
    assert e.value.status in (ERR_INVALID_ARG, ERR_BAD_STREAM), str(e.value)
    assert len(gpu_ctx.decode_streams_at(streams, 48000)[0]) == 2
    del keep


@pytest.mark.parametrize("hw,os_,cat,seed", [(romkit.HW93, D.OS93A, 0x3000, 11), (romkit.HW95, D.OS95, 0x6000, 14)], ids=["dcs93-os93a", "dcs95-os95"])
def test_extract_streams_at(gpu_ctx, hw, os_, cat, seed):
    img = romkit.RomSet(hw, os_, cat, seed, version_code=True)
    rs = D.RomSet(images=img.images)
    rs.check()
    items, pcm, first = gpu_ctx.extract_streams(rs, volume=255)
    items2, out, info, first2 = gpu_ctx.extract_streams_at(rs, 48000, volume=255)
    assert np.array_equal(items, items2) and np.array_equal(first, first2) and len(out) == len(items) > 0
    for k in range(len(items)):
        want, want_info = Q.convert(pcm[first[k]:first[k + 1]].ravel(), 48000, *table("default"))
        assert np.array_equal(out[k], want), k
        same_info(info[k], want_info, k)


def test_existing_flac_output_is_unchanged(gpu_ctx):
    """decode_streams_flac on a small list still writes the restatement's bytes (the writer is not touched by this feature)"""
    import flac_write_ref as W
    streams = list(synthetic_streams())[3:9]
    pcm, err, first = gpu_ctx.decode_streams(streams, extra_frames=2)
    for md5 in (True, False):
        out, info, got_err, _ = gpu_ctx.decode_streams_flac(streams, extra_frames=2, md5=md5)
        assert np.array_equal(got_err, err)
        assert out == [W.write(pcm[first[k]:first[k + 1]], 31250, md5)[0] for k in range(len(streams))]
