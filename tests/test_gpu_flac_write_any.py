"""The FLAC writer on streams of any length on the MI355X (dcs_flac_write_samples) against the general restatement
(tests/flac_write_any_ref.py), byte for byte, on the cases of tests/flac_write_any_cases.py: every last-block length from 1
to 40 samples and the lengths around 16s, 256 and a block, content that makes each kind of subframe and each partition
order the length allows, 300 ragged streams in one call; and dcs_decode_streams_flac_at, the chain decode -> converter ->
writer, against dcs_decode_streams_at followed by the writer.  The restatement's files are pinned to the vendored libFLAC
by tests/golden/flac_write_any_golden.json (tests/test_flac_write_any_host.py)."""
import functools

import numpy as np
import pytest

import dcsexplorer_amd as D
import flac_write_any_cases as C
import flac_write_any_ref as A
import flac_write_cases as W
import romkit
import rs_cases
from dcsexplorer_amd.api import ERR_CAPACITY, ERR_INVALID_ARG, FLAC_WRITE_INFO_DTYPE, RATE_INFO_DTYPE, DcsError, _ptr

pytestmark = pytest.mark.gpu

MD5 = pytest.mark.parametrize("md5", [True, False], ids=["md5", "nomd5"])
FIELDS = FLAC_WRITE_INFO_DTYPE.names
RATES = (48000, 44100, 4000, 65535)


@pytest.fixture(scope="module")
def ref():
    """the restatement's (bytes, info) of every case at 48 000 Hz, with and without the MD5; computed once, never changed"""
    return {(name, md5): A.write(pcm, C.RATE, md5) for name, pcm in C.cases() for md5 in (True, False)}


def same_info(got, want, what):
    assert {f: int(got[f]) for f in FIELDS} == want, what


@MD5
def test_cases_byte_for_byte(gpu_ctx, ref, md5):
    """every case in ONE call: the lengths are mostly odd, so the streams start at odd and even sample offsets alike"""
    cases = C.cases()
    starts = np.cumsum([0] + [pcm.size for _, pcm in cases])[:-1]
    assert (starts % 2 == 1).sum() > 50 and (starts % 2 == 0).sum() > 50
    out, info = gpu_ctx.flac_write_samples([pcm for _, pcm in cases], C.RATE, md5=md5)
    assert len(out) == len(cases)
    for k, (name, _) in enumerate(cases):
        want, want_info = ref[name, md5]
        assert out[k] == want, (name, len(out[k]), len(want))
        same_info(info[k], want_info, name)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 15, 17, 18, 20, 24, 4097])
def test_each_length_alone(gpu_ctx, ref, n):
    for kind in C.KINDS:
        name = "%s%d" % (kind, n)
        out, info = gpu_ctx.flac_write_samples([dict(C.cases())[name]], C.RATE)
        assert out[0] == ref[name, True][0], name
        same_info(info[0], ref[name, True][1], name)


def test_other_rates(gpu_ctx):
    for rate in C.RATES + (1,):
        out, _ = gpu_ctx.flac_write_samples([pcm for _, pcm in C.subset()], rate, md5=False)
        for got, (name, pcm) in zip(out, C.subset()):
            assert got == A.write(pcm, rate, False)[0], (name, rate)


@MD5
def test_ragged_streams_in_one_call(gpu_ctx, md5):
    pcm = C.ragged()
    want = [A.write(p, C.RATE, md5) for p in pcm]
    out, info = gpu_ctx.flac_write_samples(pcm, C.RATE, md5=md5)
    assert len(out) == len(pcm)
    for k in range(len(pcm)):
        assert out[k] == want[k][0], (k, pcm[k].size)
    for f in FIELDS:
        assert np.array_equal(info[f], np.array([w[1][f] for w in want], info[f].dtype)), f


def test_whole_frames_get_the_whole_frame_bytes(gpu_ctx):
    """flac_write_samples on streams of whole frames writes what flac_write_streams writes: nothing existing changes"""
    pcm = [x for name, x in W.cases() if name != "len35000"]
    for md5 in (True, False):
        want, want_info = gpu_ctx.flac_write_streams(pcm, md5=md5)
        out, info = gpu_ctx.flac_write_samples(pcm, 31250, md5=md5)
        assert out == want and np.array_equal(info, want_info)


def test_flac_decode_reads_what_was_written(gpu_ctx):
    """the library's own FLAC reader on the library's own files: float32(s) / 32767.f, bit for bit"""
    cases = C.cases()
    out, _ = gpu_ctx.flac_write_samples([pcm for _, pcm in cases], C.RATE)
    back = gpu_ctx.flac_decode(out)
    for (name, pcm), got in zip(cases, back):
        want = pcm.astype(np.float32) / np.float32(32767)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


# ------------------------------------------------------------------------------------------ decode -> converter -> writer

@functools.lru_cache(maxsize=None)
def mixed_streams():
    """1-frame and 17-frame streams among others, over several layouts"""
    return [(D.format_os(f), D.synth_stream(f, n, seed=0x91 + n + 8 * f, nbands=18 if f == D.FMT_93A_T1 else 16), 255, 0x50)
            for f, n in ((3, 1), (0, 17), (5, 18), (4, 60), (1, 1), (2, 17), (3, 2))]


def check_decode_streams_flac_at(ctx, streams, rate, extra_frames=2, md5=True, filter=None, at_unity=False, sequence=False):
    pcm, info_at, err, first = ctx.decode_streams_at(streams, rate, extra_frames=extra_frames, filter=filter, at_unity=at_unity,
                                                     sequence=sequence)
    want, want_info = ctx.flac_write_samples(pcm, rate, md5=md5)
    out, info, rate_info, got_err, got_first = ctx.decode_streams_flac_at(streams, rate, extra_frames=extra_frames, md5=md5, filter=filter,
                                                                          at_unity=at_unity, sequence=sequence)
    assert out == want
    assert info.dtype == FLAC_WRITE_INFO_DTYPE and np.array_equal(info, want_info)
    assert rate_info.dtype == RATE_INFO_DTYPE and rate_info.tobytes() == info_at.tobytes()
    assert np.array_equal(got_err, err) and np.array_equal(got_first, first)
    for k in range(len(streams)):                       # ... and both are the restatement's file of those samples
        assert out[k] == A.write(pcm[k], rate, md5)[0], (k, pcm[k].size)
    return pcm, out, got_err, got_first


@pytest.mark.parametrize("rate", RATES)
def test_decode_streams_flac_at(gpu_ctx, rate):
    layouts = [s for _, s in W.streams()]
    pcm, _, err, first = check_decode_streams_flac_at(gpu_ctx, layouts, rate)
    _, want_err, want_first = gpu_ctx.decode_streams(layouts, extra_frames=2)
    assert np.array_equal(err, want_err) and np.array_equal(first, want_first)
    pcm, _, err, first = check_decode_streams_flac_at(gpu_ctx, list(mixed_streams()) + layouts[::-1], rate, extra_frames=0, md5=False)
    _, want_err, want_first = gpu_ctx.decode_streams(list(mixed_streams()) + layouts[::-1], extra_frames=0)
    assert np.array_equal(err, want_err) and np.array_equal(first, want_first)
    if rate != 4000:
        assert any(p.size % 16 != 0 for p in pcm)       # (lengths the whole-frame writer would not take)


def test_decode_streams_flac_at_the_dcs_rate(gpu_ctx):
    """31 250 Hz: without at_unity the bytes are decode_streams_flac's; with it the writer's on the unity-converted samples"""
    streams = [s for _, s in W.streams()] + list(mixed_streams())
    want, want_info, want_err, want_first = gpu_ctx.decode_streams_flac(streams, extra_frames=2)
    out, info, rate_info, err, first = gpu_ctx.decode_streams_flac_at(streams, 31250, extra_frames=2)
    assert out == want and np.array_equal(info, want_info) and np.array_equal(err, want_err) and np.array_equal(first, want_first)
    assert np.array_equal(rate_info["nIn"], rate_info["nOut"])
    check_decode_streams_flac_at(gpu_ctx, streams, 31250, at_unity=True)
    check_decode_streams_flac_at(gpu_ctx, streams, 31250, md5=False)


def test_decode_streams_flac_at_as_a_sequence(gpu_ctx):
    seq = [(D.format_os(3), D.synth_stream(3, n, seed=0x51 + n), 255, lv) for n, lv in ((17, 0x64), (1, 0x50), (33, 0x64), (2, 0x40))]
    check_decode_streams_flac_at(gpu_ctx, seq, 44100, sequence=True)
    check_decode_streams_flac_at(gpu_ctx, seq, 48000, extra_frames=3, md5=False, sequence=True)


def test_decode_streams_flac_at_with_another_filter(gpu_ctx):
    table = rs_cases.tables()["fastest"]
    streams = list(mixed_streams())
    pcm, _, _, _ = check_decode_streams_flac_at(gpu_ctx, streams, 48000, filter=table)
    plain = gpu_ctx.decode_streams_at(streams, 48000, extra_frames=2)[0]
    assert any(not np.array_equal(a, b) for a, b in zip(pcm, plain))     # (the table was used)


@pytest.mark.parametrize("hw,os_,cat,seed", [(romkit.HW93, D.OS93A, 0x3000, 11), (romkit.HW95, D.OS95, 0x6000, 14)], ids=["dcs93-os93a", "dcs95-os95"])
def test_extract_streams_flac_at(gpu_ctx, hw, os_, cat, seed):
    img = romkit.RomSet(hw, os_, cat, seed, version_code=True)
    rs = D.RomSet(images=img.images)
    rs.check()
    items, pcm, rate_info, first = gpu_ctx.extract_streams_at(rs, 48000, volume=255)
    items2, out, info, rate_info2, first2 = gpu_ctx.extract_streams_flac_at(rs, 48000, volume=255)
    assert np.array_equal(items, items2) and np.array_equal(first, first2) and len(out) == len(items) > 0
    assert rate_info2.tobytes() == rate_info.tobytes()
    want, want_info = gpu_ctx.flac_write_samples(pcm, 48000)
    assert out == want and np.array_equal(info, want_info)
    for k in range(len(items)):
        assert out[k] == A.write(pcm[k], 48000, True)[0], k


def test_capacity_protocol(gpu_ctx, ref):
    """outCap one byte short: DCS_ERR_CAPACITY with outOffsets and info filled; a second call with that capacity succeeds"""
    names = ("tone17", "const3", "noise4097")
    cases = dict(C.cases())
    arrs = [cases[n] for n in names]
    pcm = np.concatenate(arrs)
    offs = np.concatenate(([0], np.cumsum([a.size for a in arrs]))).astype(np.uint64)
    want = [ref[n, True][0] for n in names]
    need = sum(map(len, want))
    L = gpu_ctx.L
    for cap, status in ((need - 1, ERR_CAPACITY), (0, ERR_CAPACITY), (need, 0)):
        out = np.full(need + 8, 0xAA, np.uint8)
        out_offs = np.zeros(4, np.uint64)
        info = np.zeros(3, FLAC_WRITE_INFO_DTYPE)
        st = L.dcs_flac_write_samples(gpu_ctx.h, _ptr(pcm), _ptr(offs), 3, C.RATE, D.FLAC_MD5, _ptr(out), cap, _ptr(out_offs), _ptr(info))
        assert st == status, cap
        assert list(out_offs) == [0] + list(np.cumsum([len(w) for w in want])), cap
        assert [int(b) for b in info["nBytes"]] == [len(w) for w in want]
        if status == 0:
            assert out[:need].tobytes() == b"".join(want) and (out[need:] == 0xAA).all()
        else:
            assert (out == 0xAA).all()                  # (nothing is written into a buffer that is too small)
    # the same through the decoder: the error words and the converter's figures come down on both statuses
    streams = [s for _, s in W.streams()][:2]
    good, good_info, good_rate, good_err, _ = gpu_ctx.decode_streams_flac_at(streams, 48000, extra_frames=2)
    refs, keep = D.api._stream_refs(streams)
    need = sum(map(len, good))
    for cap, status in ((need - 1, ERR_CAPACITY), (need, 0)):
        out = np.full(need + 8, 0xAA, np.uint8)
        out_offs = np.zeros(3, np.uint64)
        info = np.zeros(2, FLAC_WRITE_INFO_DTYPE)
        rate_info = np.zeros(2, RATE_INFO_DTYPE)
        err = np.full(70, 0xFFFFFFFF, np.uint32)
        st = L.dcs_decode_streams_flac_at(gpu_ctx.h, refs, 2, 2, 48000, None, D.FLAC_MD5, _ptr(out), cap, _ptr(out_offs), _ptr(info),
                                          _ptr(rate_info), _ptr(err))
        assert st == status, cap
        assert int(out_offs[2]) == need and np.array_equal(info, good_info) and rate_info.tobytes() == good_rate.tobytes()
        assert np.array_equal(err, good_err)
        if status == 0:
            assert out[:need].tobytes() == b"".join(good) and (out[need:] == 0xAA).all()
        else:
            assert (out == 0xAA).all()
    assert L.dcs_decode_streams_flac_at(gpu_ctx.h, refs, 2, 2, 48000, None, 0, None, 0, _ptr(out_offs), None, None, None) == ERR_CAPACITY
    del keep


def test_refused_calls_name_their_reason_and_leave_the_context_usable(gpu_ctx, ref):
    good = dict(C.cases())["tone17"]
    for bad, rate, word in (([good, np.zeros(0, np.int16)], 48000, "stream 1"), ([good], 0, "rate"), ([good], 65536, "rate")):
        with pytest.raises(DcsError) as e:
            gpu_ctx.flac_write_samples(bad, rate)
        assert e.value.status == ERR_INVALID_ARG and word in str(e.value), str(e.value)
        assert gpu_ctx.flac_write_samples([good], C.RATE)[0][0] == ref["tone17", True][0]
    # the whole-frame calls keep their refusals
    for n in (239, 241, 4096):
        with pytest.raises(DcsError) as e:
            gpu_ctx.flac_write_streams([np.zeros(n, np.int16)])
        assert e.value.status == ERR_INVALID_ARG and "whole frames" in str(e.value)
    streams = [W.streams()[3][1], W.streams()[3][1]]
    for rate, word in ((3999, "rate"), (65536, "rate")):
        with pytest.raises(DcsError) as e:
            gpu_ctx.decode_streams_flac_at(streams, rate)
        assert e.value.status == ERR_INVALID_ARG and word in str(e.value), str(e.value)
        check_decode_streams_flac_at(gpu_ctx, streams[:1], 48000)
    refs, keep = D.api._stream_refs(streams)
    out_offs = np.zeros(3, np.uint64)
    st = gpu_ctx.L.dcs_decode_streams_flac_at(gpu_ctx.h, refs, 2, 2, 48000, None, 8, None, 0, _ptr(out_offs), None, None, None)
    assert st == ERR_INVALID_ARG and b"unknown flags" in gpu_ctx.L.dcs_last_error(gpu_ctx.h)
    with pytest.raises(DcsError) as e:
        gpu_ctx.decode_streams_flac_at(streams, 48000, extra_frames=1, sequence=True)
    assert e.value.status == ERR_INVALID_ARG and "dcs_decode_streams_flac_at" in str(e.value) and "2 extra frames" in str(e.value)
    check_decode_streams_flac_at(gpu_ctx, streams, 44100, sequence=True)
    del keep
