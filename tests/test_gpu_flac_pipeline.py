"""FLAC as a pipeline output on the MI355X (DCS_PIPE_FLAC, dcs_pipeline_collect_flac): every pipeline shape against the PCM
pipeline of the same shape, dcs_decode_streams_flac and the numpy restatement (tests/flac_write_ref.py), byte for byte; the
scan across streams at the counts where a wavefront step, a round of 256 and the carry between rounds can go wrong; the copy
whose length only the device knows, at every residue of the total modulo 16 that a handful of lists reach; the stream heads
at every byte alignment; the collect protocol.  The lists are small on purpose."""
import ctypes
import threading

import numpy as np
import pytest

import dcsexplorer_amd as D
import flac_write_cases as C
import flac_write_ref as R
from dcsexplorer_amd.api import (ERR_BAD_STREAM, ERR_INVALID_ARG, FLAC_WRITE_INFO_DTYPE, DcsError, PipelineFlacResult, PipelineResult,
                                 _ptr, _stream_refs)
from util import ALL_FORMATS, make_stream, os_for

pytestmark = pytest.mark.gpu

FIELDS = FLAC_WRITE_INFO_DTYPE.names
SHAPES = pytest.mark.parametrize("flags", [0, 1, 3, 7], ids=["host", "index", "pack", "plan"])
MD5 = pytest.mark.parametrize("md5", [True, False], ids=["md5", "nomd5"])
RAGGED = 1                                              # LISTS[RAGGED]: ten streams of 1 to 60 frames
TRUNCATED = 4                                           # LISTS[TRUNCATED]: the list the device planner hands back


def synth(fmt, frames, seed):
    return (D.format_os(fmt), D.synth_stream(fmt, frames, seed=seed, nbands=18 if fmt == D.FMT_93A_T1 else 16), 255, 0x64)


def make_lists():
    """(streams, extra_frames) of the five lists"""
    six = [s for _, s in C.streams()]
    more = [(D.format_os(f), D.synth_stream(f, n, seed=0x77 + n), 255, 0x50) for f, n in ((3, 1), (0, 17), (5, 18), (4, 60))]
    one_frame = [synth(k % 6, 1, 0x3000 + k) for k in range(300)]
    cut = six[:5] + [(six[5][0], six[5][1][:len(six[5][1]) // 2], six[5][2], six[5][3])]
    return [(six, 0), (six + more, 1), ([six[2]], 2), (one_frame, 0), (cut, 2)]


LISTS = make_lists()


def pipeline(ctx, flags, flac=False, md5=True, depth=3):
    return ctx.pipeline(depth, index_on_device=bool(flags & 1), pack_on_device=bool(flags & 2), plan_on_device=bool(flags & 4), flac=flac, md5=md5)


def through(pipe, lists, collect):
    """the lists submitted from a thread of its own -- submit blocks once `depth` lists are between submit and collect, so more
    lists than that cannot all be submitted ahead of the first collect from one thread -- and collected here, the first collect
    only once as many lists as the pipeline holds are in: others are in flight behind the one collected"""
    depth, n_in = 3, [0]
    failed = []

    def submit():
        try:
            for streams, extra in lists:
                pipe.submit(streams, extra_frames=extra)
                n_in[0] += 1
        except Exception as e:                          # noqa: BLE001
            failed.append(e)

    t = threading.Thread(target=submit)
    t.start()
    while n_in[0] < min(depth, len(lists)) and t.is_alive():
        pass
    out = []
    for _ in lists:
        out.append(collect() + (pipe.last_path,))
    t.join()
    assert not failed, failed
    return out


@pytest.fixture(scope="module")
def want(gpu_ctx):
    """per list: decode_streams' (pcm, err, first), the restatement's files of that PCM and decode_streams_flac's (out, info),
    with and without the MD5; computed once, never changed"""
    out = []
    for streams, extra in LISTS:
        pcm, err, first = gpu_ctx.decode_streams(streams, extra_frames=extra)
        entry = dict(err=err.copy(), first=first.copy())
        for md5 in (True, False):
            files = [R.write(pcm[first[k]:first[k + 1]], 31250, md5) for k in range(len(streams))]
            sync_out, sync_info, sync_err, sync_first = gpu_ctx.decode_streams_flac(streams, extra_frames=extra, md5=md5)
            assert np.array_equal(sync_err, err) and np.array_equal(sync_first, first)
            entry[md5] = dict(files=[f for f, _ in files], infos=[i for _, i in files], sync_out=sync_out, sync_info=sync_info)
        out.append(entry)
    return out


_PCM_PIPE = {}


def pcm_pipeline_results(ctx, flags):
    """(err, first, path) of every list through a PCM pipeline of these flags; once per shape"""
    if flags not in _PCM_PIPE:
        pipe = pipeline(ctx, flags)
        res = through(pipe, LISTS, lambda: tuple(np.array(x) for x in pipe.collect()[1:3]))
        pipe.close()
        _PCM_PIPE[flags] = res
    return _PCM_PIPE[flags]


def check_list(got, w, md5, what):
    out, info, err, first = got[:4]
    assert np.array_equal(err, w["err"]) and np.array_equal(first, w["first"]), what
    assert np.array_equal(info, w[md5]["sync_info"]), what
    assert len(out) == len(w[md5]["files"]), what
    for k, (a, b, c) in enumerate(zip(out, w[md5]["sync_out"], w[md5]["files"])):
        assert a == b, (what, k, "decode_streams_flac", len(a), len(b))
        assert a == c, (what, k, "restatement", len(a), len(c))
    for f in FIELDS:
        assert [int(x) for x in info[f]] == [i[f] for i in w[md5]["infos"]], (what, f)


@SHAPES
@MD5
def test_every_shape_byte_for_byte(gpu_ctx, want, flags, md5):
    pcm_side = pcm_pipeline_results(gpu_ctx, flags)
    pipe = pipeline(gpu_ctx, flags, flac=True, md5=md5)
    got = through(pipe, LISTS, pipe.collect_flac)
    pipe.close()
    for i, (g, w, p) in enumerate(zip(got, want, pcm_side)):
        check_list(g, w, md5, (flags, md5, i))
        assert np.array_equal(g[2], p[0]) and np.array_equal(g[3], p[1]), (flags, i)
        if flags == 7:
            # the truncated list, and no other, took the host-planned fallback: in the PCM pipeline as here
            assert (g[-1] == 7) == (i != TRUNCATED) and (p[-1] == 7) == (i != TRUNCATED), (i, g[-1], p[-1])


@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 1000])
def test_scan_across_streams(gpu_ctx, n):
    """dcs_flac_write_streams is the same queueing function: one-frame streams dealt from the pool, so that every stream's
    base is the sum of many sizes"""
    _, pool, _ = C.shapes()[1]
    files = [R.write(p, 31250, True) for p in pool]
    index = np.random.default_rng([C.SEED, 31, n]).integers(0, len(pool), n)
    pcm = np.concatenate([pool[i] for i in index])
    offs = (np.arange(n + 1) * C.FRAME).astype(np.uint64)
    cap = n * D.flac_write_bound(C.FRAME)
    out, out_offs, info = np.zeros(cap, np.uint8), np.zeros(n + 1, np.uint64), np.zeros(n, FLAC_WRITE_INFO_DTYPE)
    st = gpu_ctx.L.dcs_flac_write_streams(gpu_ctx.h, _ptr(pcm), _ptr(offs), n, 31250, D.FLAC_MD5, _ptr(out), cap, _ptr(out_offs), _ptr(info))
    assert st == 0
    sizes = [len(files[i][0]) for i in index]
    assert [int(x) for x in out_offs] == [0] + [int(x) for x in np.cumsum(sizes)]
    assert out[:int(out_offs[n])].tobytes() == b"".join(files[i][0] for i in index)
    for f in FIELDS:
        assert [int(x) for x in info[f]] == [files[i][1][f] for i in index], f


RESIDUE_SEEDS = (11, 2, 28, 3, 4, 5, 14, 0, 22)         # picked with the restatement: their lists' totals modulo 16 are 0 to 8


def residue_list(seed):
    return [synth(seed % 6, 1 + seed % 3, 0x9000 + seed), synth(3, 2, 0x9900 + seed)]


def test_length_driven_copy(gpu_ctx, oracle):
    """the FLAC bytes come down by a copy whose length is a word on the device, rounded up to 16: lists whose totals cover
    nine residues modulo 16, 0 among them, checked to their last byte"""
    lists, files = [], []
    for seed in RESIDUE_SEEDS:
        lst = residue_list(seed)
        pcm = [np.ascontiguousarray(oracle.decode(os_, vol, [s], [lvl], (s[0] << 8) | s[1]), np.int16).ravel() for os_, s, vol, lvl in lst]
        lists.append((lst, 0))
        files.append([R.write(p, 31250, True)[0] for p in pcm])
    totals = [sum(map(len, f)) for f in files]
    residues = {t % 16 for t in totals}
    assert len(residues) >= 8 and 0 in residues, sorted(residues)
    pipe = pipeline(gpu_ctx, 7, flac=True)
    got = through(pipe, lists, pipe.collect_flac)
    pipe.close()
    for g, f, total in zip(got, files, totals):
        assert len(b"".join(g[0])) == total and int(g[1]["nBytes"].sum()) == total
        assert g[0] == f, total % 16


def test_heads_at_every_alignment(gpu_ctx, want):
    """the 42 bytes in front of a stream are stored byte by byte wherever the stream begins: in the ragged list the bases take
    all four alignments, and neither a head nor the four bytes on either side of it differ"""
    w = want[RAGGED][True]
    sizes = [len(f) for f in w["files"]]
    bases = [int(b) for b in np.concatenate(([0], np.cumsum(sizes)))[:-1]]
    assert {b % 4 for b in bases} == {0, 1, 2, 3}, bases
    pipe = pipeline(gpu_ctx, 7, flac=True)
    pipe.submit(*LISTS[RAGGED][:1], extra_frames=LISTS[RAGGED][1])
    out = pipe.collect_flac()[0]
    pipe.close()
    got, ref = b"".join(out), b"".join(w["files"])
    assert len(got) == len(ref)
    for k, b in enumerate(bases):
        assert out[k][:42] == w["files"][k][:42], k
        lo, hi = max(b - 4, 0), min(b + 46, len(ref))
        assert got[lo:hi] == ref[lo:hi], (k, b % 4)


def test_wrong_collect_call_leaves_the_list(gpu_ctx, want):
    streams, extra = LISTS[2]
    for flac in (True, False):
        pipe = pipeline(gpu_ctx, 7, flac=flac)
        pipe.submit(streams, extra_frames=extra)
        if flac:
            assert gpu_ctx.L.dcs_pipeline_collect(pipe.h, ctypes.byref(PipelineResult())) == ERR_INVALID_ARG
            with pytest.raises(DcsError) as e:
                pipe.collect()
            assert e.value.status == ERR_INVALID_ARG
            check_list(pipe.collect_flac(), want[2], True, "after the wrong call")
        else:
            assert gpu_ctx.L.dcs_pipeline_collect_flac(pipe.h, ctypes.byref(PipelineFlacResult())) == ERR_INVALID_ARG
            with pytest.raises(DcsError) as e:
                pipe.collect_flac()
            assert e.value.status == ERR_INVALID_ARG
            pcm, err, first, _, _ = pipe.collect()
            assert np.array_equal(err, want[2]["err"]) and np.array_equal(first, want[2]["first"]) and pcm.shape[0] == first[-1]
        pipe.close()


def test_flags_refused(gpu_ctx):
    h = ctypes.c_void_p()
    for flags in (D.PIPE_FLAC_MD5, D.PIPE_FLAC_MD5 | 7, 32, 32 | D.PIPE_FLAC, 64 | D.PIPE_FLAC | D.PIPE_FLAC_MD5):
        assert gpu_ctx.L.dcs_pipeline_create(gpu_ctx.h, 2, flags, ctypes.byref(h)) == ERR_INVALID_ARG, flags
        assert not h.value
    node = ctypes.c_void_p()
    ids = (ctypes.c_int * 1)(0)
    for flags in (D.PIPE_FLAC, D.PIPE_FLAC | D.PIPE_FLAC_MD5 | 7):
        assert gpu_ctx.L.dcs_node_create(ids, 1, 2, flags, ctypes.byref(node)) == ERR_INVALID_ARG, flags
        assert not node.value


@pytest.mark.parametrize("flags", [0, 7], ids=["host", "plan"])
def test_bad_list_and_the_one_behind_it(gpu_ctx, want, flags):
    """a list with a zero-frame stream fails by itself; a result copied after its collect is still right after the next"""
    streams, extra = LISTS[0]
    bad = streams[:2] + [(streams[0][0], bytes(24), 255, 0x64)] + streams[2:]
    pipe = pipeline(gpu_ctx, flags, flac=True)
    pipe.submit(streams, extra_frames=extra)
    pipe.submit(bad, extra_frames=extra)
    pipe.submit(*LISTS[2][:1], extra_frames=LISTS[2][1])
    first_result = pipe.collect_flac()
    with pytest.raises(DcsError) as e:
        pipe.collect_flac()
    assert e.value.status == ERR_BAD_STREAM
    check_list(pipe.collect_flac(), want[2], True, "behind the bad list")
    check_list(first_result, want[0], True, "copied before two more collects")
    pipe.close()


def flac_behind_attempts(gpu_ctx, oracle, hard, behind):
    """`hard` (extra_frames=2), then `behind`, through a FLAC pipeline with the planner on the device and 8 frames per wavefront:
    hard's FLAC bytes against decode_streams_flac on the same list and against the restatement of the oracle's PCM, its error
    words zero -> (hard's path, behind's result with its path last)"""
    files = [R.write(oracle.decode(o, v, [s], [l], ((s[0] << 8) | s[1]) + 2), 31250, True)[0] for o, s, v, l in hard]
    try:
        gpu_ctx.set_frames_per_wave(8)
        sync_out, sync_info, sync_err, sync_first = gpu_ctx.decode_streams_flac(hard, extra_frames=2)
        pipe = pipeline(gpu_ctx, 7, flac=True)
        pipe.submit(hard, extra_frames=2)
        pipe.submit(behind[0], extra_frames=behind[1])
        out, info, err, first = pipe.collect_flac()[:4]
        path = pipe.last_path
        got_behind = pipe.collect_flac() + (pipe.last_path,)
        pipe.close()
    finally:
        gpu_ctx.set_frames_per_wave(0)
    assert len(out) == len(hard) and np.array_equal(first, sync_first) and np.array_equal(info, sync_info)
    for k, (a, b, c) in enumerate(zip(out, sync_out, files)):
        assert a == b, (k, "decode_streams_flac", len(a), len(b))
        assert a == c, (k, "restatement", len(a), len(c))
    assert not err.any() and not sync_err.any()
    return path, got_behind


def test_flac_ending_behind_a_list_planned_again(gpu_ctx, oracle, want):
    """the list of test_large_frames_are_planned_again_on_the_device_with_fewer_frames_per_chunk (tests/test_gpu_corpus.py): the
    first attempt's FLAC buffers are dropped, the list is planned again on the device and its FLAC ending queued a second time;
    the ordinary list behind it is what it is alone"""
    hard = [(os_for(f, f & 1), make_stream(f, 60 + f, seed=67000 + f, profile=4, nbands=10), 255, 0x64) for f in (0, 1, 3)]
    hard += [(os_for(f, 1), make_stream(f, 40, seed=67100 + f), 255, 0x64) for f in ALL_FORMATS]
    path, behind = flac_behind_attempts(gpu_ctx, oracle, hard, LISTS[0])
    assert path == 7
    check_list(behind, want[0], True, "behind the list planned again")
    assert behind[-1] == 7


def test_flac_ending_behind_a_list_handed_back(gpu_ctx, oracle):
    """the saturated list of tests/test_gpu_corpus.py, which overflows the bit pool with six and with four frames per chunk too:
    three attempts' FLAC endings are abandoned, then the host-planned path writes the list's FLAC; the easy list behind it stays
    on the device"""
    hard = [(os_for(f, f & 1), make_stream(f, 48 + f, seed=66000 + f, profile=4), 255, 0x64) for f in ALL_FORMATS]
    easy = [(os_for(f, f & 1), make_stream(f, 48 + f, seed=66100 + f), 255, 0x64) for f in ALL_FORMATS]
    path, behind = flac_behind_attempts(gpu_ctx, oracle, hard, (easy, 2))
    assert path == 0
    assert behind[-1] == 7
    alone_out, alone_info, alone_err, alone_first = gpu_ctx.decode_streams_flac(easy, extra_frames=2)
    assert behind[0] == alone_out and np.array_equal(behind[1], alone_info)
    assert np.array_equal(behind[2], alone_err) and np.array_equal(behind[3], alone_first)


def test_destroy_with_uncollected_lists(gpu_ctx):
    pipe = pipeline(gpu_ctx, 7, flac=True)
    for streams, extra in LISTS[:3]:
        pipe.submit(streams, extra_frames=extra)
    pipe.close()
    assert pipe.h is None


def test_zz_context_still_usable(gpu_ctx, want):
    """after all of the above (the tests of a module run in the order they are written)"""
    for (streams, extra), w in zip(LISTS, want):
        pcm, err, first = gpu_ctx.decode_streams(streams, extra_frames=extra)
        assert np.array_equal(err, w["err"]) and np.array_equal(first, w["first"])
        out, info, err2, first2 = gpu_ctx.decode_streams_flac(streams, extra_frames=extra)
        assert out == w[True]["sync_out"] and np.array_equal(info, w[True]["sync_info"]) and np.array_equal(err2, err)
        assert out == [R.write(pcm[first[k]:first[k + 1]], 31250, True)[0] for k in range(len(streams))]
