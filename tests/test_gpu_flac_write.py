"""The FLAC writer on the MI355X (dcs_flac_write_streams, dcs_decode_streams_flac) against its numpy restatement
(tests/flac_write_ref.py), byte for byte, on the cases of tests/flac_write_cases.py: the block lengths that change the
frame header's form, frame numbers coded in one, two and three bytes, content that makes each kind of subframe, 300 ragged
streams in one call and 70 000 one-frame streams, more blocks than a grid's y dimension holds.  The restatement's files are
pinned to the vendored libFLAC by tests/golden/flac_write_golden.json (tests/test_flac_write_host.py)."""
import ctypes

import numpy as np
import pytest

import dcsexplorer_amd as D
import flac_write_cases as C
import flac_write_ref as R
import romkit
from dcsexplorer_amd.api import ERR_CAPACITY, ERR_INVALID_ARG, FLAC_WRITE_INFO_DTYPE, DcsError, _ptr

pytestmark = pytest.mark.gpu

MD5 = pytest.mark.parametrize("md5", [True, False], ids=["md5", "nomd5"])
FIELDS = FLAC_WRITE_INFO_DTYPE.names


@pytest.fixture(scope="module")
def ref():
    """the restatement's (bytes, info) of every case, with and without the MD5; computed once, never changed"""
    return {(name, md5): R.write(pcm, 31250, md5) for name, pcm in C.cases() for md5 in (True, False)}


def same_info(got, want, what):
    assert {f: int(got[f]) for f in FIELDS} == want, what


@MD5
def test_cases_byte_for_byte(gpu_ctx, ref, md5):
    """every case in ONE call, so that each stream starts at another offset in the PCM and in the output"""
    cases = C.cases()
    out, info = gpu_ctx.flac_write_streams([pcm for _, pcm in cases], md5=md5)
    assert len(out) == len(cases)
    for k, (name, _) in enumerate(cases):
        want, want_info = ref[name, md5]
        assert out[k] == want, (name, len(out[k]), len(want))
        same_info(info[k], want_info, name)


def test_each_case_alone_and_other_rates(gpu_ctx, ref):
    cases = dict(C.cases())
    for name in ("len1", "len17", "len18", "spike", "synth2"):
        out, info = gpu_ctx.flac_write_streams([cases[name]])
        assert out[0] == ref[name, True][0], name
    for rate in (1, 8000, 44100, 65535):
        out, info = gpu_ctx.flac_write_streams([cases["len18"], cases["segments"]], rate=rate, md5=False)
        for got, name in zip(out, ("len18", "segments")):
            assert got == R.write(cases[name], rate, False)[0], (name, rate)


@MD5
@pytest.mark.parametrize("shape", [0, 1], ids=["ragged300", "one_frame_70000"])
def test_many_streams_in_one_call(gpu_ctx, shape, md5):
    name, pool, index = C.shapes()[shape]
    want = [R.write(p, 31250, md5) for p in pool]
    out, info = gpu_ctx.flac_write_streams([pool[i] for i in index], md5=md5)
    assert len(out) == len(index)
    for k, i in enumerate(index):
        assert out[k] == want[i][0], (name, k)
    for f in FIELDS:
        assert np.array_equal(info[f], np.array([want[i][1][f] for i in index], info[f].dtype)), (name, f)


def test_flac_decode_reads_what_was_written(gpu_ctx, ref):
    """the library's own FLAC reader on the library's own files: float32(s) / 32767.f, bit for bit"""
    cases = C.cases()
    out, _ = gpu_ctx.flac_write_streams([pcm for _, pcm in cases])
    back = gpu_ctx.flac_decode(out)
    for (name, pcm), got in zip(cases, back):
        want = pcm.astype(np.float32) / np.float32(32767)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


def test_flac_decode_at_every_alignment(gpu_ctx, ref):
    """the zeros63 cases behind 0..3 files of 249 bytes: every alignment of their frames in the uploaded bytes"""
    cases = dict(C.cases())
    filler = ref["len1", True][0]
    assert len(filler) % 4 == 1
    for name in ("zeros63_2", "zeros63_4", "zeros63_8"):
        want = cases[name].astype(np.float32) / np.float32(32767)
        for lead in range(4):
            back = gpu_ctx.flac_decode([filler] * lead + [ref[name, True][0]])
            assert np.array_equal(back[-1].view(np.uint32), want.view(np.uint32)), (name, lead)


def check_decode_streams_flac(ctx, streams, extra_frames, md5):
    pcm, err, first = ctx.decode_streams(streams, extra_frames=extra_frames)
    per_stream = [pcm[first[k]:first[k + 1]] for k in range(len(streams))]
    want, want_info = ctx.flac_write_streams(per_stream, md5=md5)
    out, info, got_err, got_first = ctx.decode_streams_flac(streams, extra_frames=extra_frames, md5=md5)
    assert out == want
    assert np.array_equal(info, want_info)
    assert np.array_equal(got_err, err) and np.array_equal(got_first, first)
    for k in range(len(streams)):                       # ... and both are the restatement's file of that PCM
        assert out[k] == R.write(per_stream[k], 31250, md5)[0], k


@pytest.mark.parametrize("fmt", range(6))
def test_decode_streams_flac_each_layout(gpu_ctx, fmt):
    check_decode_streams_flac(gpu_ctx, [C.streams()[fmt][1]], 2, True)


def test_decode_streams_flac_mixed_list(gpu_ctx):
    streams = [s for _, s in C.streams()]
    more = [(D.format_os(f), D.synth_stream(f, n, seed=0x77 + n), 255, 0x50) for f, n in ((3, 1), (0, 17), (5, 18), (4, 60))]
    check_decode_streams_flac(gpu_ctx, streams + more + streams[::-1], 0, False)
    check_decode_streams_flac(gpu_ctx, more + streams, 1, True)


def damaged_streams():
    """a 1994+ stream with three seeded bit flips, 64 times; the ones the index pass cuts short"""
    os_, s, vol, lvl = C.streams()[3][1]
    out = []
    for seed in range(64):
        r = np.random.default_rng([C.SEED, seed])
        b = bytearray(s)
        for at in r.integers(16 * 8, len(b) * 8, 3):
            b[at >> 3] ^= 1 << (at & 7)
        cand = bytes(b) + bytes(1024)
        _, info = D.index_stream(os_, cand)
        if info.nValidFrames < info.nFrames:
            out.append((os_, cand, vol, lvl))
    return out


def test_decode_streams_flac_keeps_a_stream_with_a_fatal_frame(gpu_ctx):
    """a stream with a fatal frame is written as the PCM the decoder produced; the error words say what happened"""
    streams = damaged_streams() + [C.streams()[4][1]]
    pcm, err, first = gpu_ctx.decode_streams(streams, extra_frames=2)
    fatal = [k for k in range(len(streams)) if (err[first[k]:first[k + 1]] & D.FRAME_FATAL).any()]
    assert fatal and not err[first[-2]:].any()
    out, info, got_err, _ = gpu_ctx.decode_streams_flac(streams, extra_frames=2)
    assert np.array_equal(got_err, err)
    assert out == [R.write(pcm[first[k]:first[k + 1]], 31250, True)[0] for k in range(len(streams))]


@pytest.mark.parametrize("hw,os_,cat,seed", [(romkit.HW93, D.OS93A, 0x3000, 11), (romkit.HW95, D.OS95, 0x6000, 14)], ids=["dcs93-os93a", "dcs95-os95"])
def test_extract_streams_flac(gpu_ctx, hw, os_, cat, seed):
    img = romkit.RomSet(hw, os_, cat, seed, version_code=True)
    rs = D.RomSet(images=img.images)
    rs.check()
    items, pcm, first = gpu_ctx.extract_streams(rs, volume=255)
    items2, out, info, first2 = gpu_ctx.extract_streams_flac(rs, volume=255)
    assert np.array_equal(items, items2) and np.array_equal(first, first2) and len(out) == len(items) > 0
    for k in range(len(items)):
        want, want_info = R.write(pcm[first[k]:first[k + 1]], 31250, True)
        assert out[k] == want, k
        same_info(info[k], want_info, k)


def test_capacity_protocol(gpu_ctx, ref):
    """outCap one byte short: DCS_ERR_CAPACITY with outOffsets and info filled; a second call with that capacity succeeds"""
    names = ("len18", "silence", "white")
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
        st = L.dcs_flac_write_streams(gpu_ctx.h, _ptr(pcm), _ptr(offs), 3, 31250, D.FLAC_MD5, _ptr(out), cap, _ptr(out_offs), _ptr(info))
        assert st == status, cap
        assert list(out_offs) == [0] + list(np.cumsum([len(w) for w in want])), cap
        assert [int(b) for b in info["nBytes"]] == [len(w) for w in want]
        if status == 0:
            assert out[:need].tobytes() == b"".join(want) and (out[need:] == 0xAA).all()
        else:
            assert (out == 0xAA).all()                  # (nothing is written into a buffer that is too small)
    assert L.dcs_flac_write_streams(gpu_ctx.h, _ptr(pcm), _ptr(offs), 3, 31250, D.FLAC_MD5, None, 0, _ptr(out_offs), None) == ERR_CAPACITY
    # the same through the decoder
    streams = [s for _, s in C.streams()][:2]
    good, _, _, _ = gpu_ctx.decode_streams_flac(streams, extra_frames=2)
    refs, keep = D.api._stream_refs(streams)
    need = sum(map(len, good))
    out = np.zeros(need, np.uint8)
    out_offs = np.zeros(3, np.uint64)
    err = np.zeros(70, np.uint32)
    assert L.dcs_decode_streams_flac(gpu_ctx.h, refs, 2, 2, D.FLAC_MD5, _ptr(out), need - 1, _ptr(out_offs), None, _ptr(err)) == ERR_CAPACITY
    assert int(out_offs[2]) == need
    assert L.dcs_decode_streams_flac(gpu_ctx.h, refs, 2, 2, D.FLAC_MD5, _ptr(out), need, _ptr(out_offs), None, _ptr(err)) == 0
    assert out.tobytes() == b"".join(good)


def test_refused_call_leaves_the_context_usable(gpu_ctx, ref):
    cases = dict(C.cases())
    good = cases["len17"]
    for bad, rate, word in (([good, np.zeros(241, np.int16)], 31250, "stream 1"), ([np.zeros(0, np.int16), good], 31250, "stream 0"),
                            ([good], 0, "rate"), ([good], 65536, "rate")):
        with pytest.raises(DcsError) as e:
            gpu_ctx.flac_write_streams(bad, rate=rate)
        assert e.value.status == ERR_INVALID_ARG and word in str(e.value), str(e.value)
        out, _ = gpu_ctx.flac_write_streams([good])
        assert out[0] == ref["len17", True][0]
    refs, keep = D.api._stream_refs([C.streams()[0][1]])
    out_offs = np.zeros(2, np.uint64)
    for flags, extra in ((4, 0), (D.FLAC_SEQUENCE, 1)):
        assert gpu_ctx.L.dcs_decode_streams_flac(gpu_ctx.h, refs, 1, extra, flags, None, 0, _ptr(out_offs), None, None) == ERR_INVALID_ARG
    check_decode_streams_flac(gpu_ctx, [C.streams()[0][1]], 2, True)
