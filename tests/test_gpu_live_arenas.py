"""The live decoder's arenas and the other grow-only buffers outside the context's cache (GrowBuf, dcs_cache.h), on a real MI355X:
the paths no other test reaches -- arenas that grow past their first size and are then used by small calls, hand-off words that grow
twice under chains that cross every chunk boundary, a refused call in front of a good one, what one blob leaves behind a shorter
one's end, the cache's byte counts next to all of it, and the index inputs that stay resident.  Against the oracle, or the committed
goldens where there are any; one Context per case."""
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
from graph_ref import graph_ref
from mixer_ref import build_mix_batch
from util import ALL_FORMATS, make_stream, os_for

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FMT94 = [D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3]
ZC = {"default": None, "always-copy": ("0", "0"), "never-copy": ("1000000", "1000000")}


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d values differ in %d rows; first at %s: got %d want %d"
                             % (what, len(bad), len(set(bad[:, 0])), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _window(b, lo, n, first_prev=D.PREV_NONE):
    """jobs [lo, lo + n) of a batch of single-source chains as a list of their own (lo: a stream's first job unless first_prev
    names an external tail) -> (srcs, jobs)"""
    jobs = b["jobs"][lo:lo + n].copy()
    assert (jobs["nSrc"] == 1).all()
    s0 = int(jobs["firstSrc"].min())
    s1 = int(jobs["firstSrc"].max()) + 1
    jobs["firstSrc"] -= s0
    link = jobs["prev"] != D.PREV_NONE
    jobs["prev"][link] -= lo
    jobs["prev"][0] = first_prev
    assert ((jobs["prev"][1:] == D.PREV_NONE) | (jobs["prev"][1:] < n)).all()
    return b["srcs"][s0:s1], jobs


@pytest.fixture(scope="module")
def long_lists(oracle):
    """36 synthetic 1994+ streams of 250 frames as one batch, with the oracle's PCM and every frame's tail (computed once)"""
    streams = [(os_for(FMT94[k % 3], k), make_stream(FMT94[k % 3], 250, seed=52000 + k, profile=k % 4), 255 - 3 * k, 0x64) for k in range(36)]
    b = D.build_stream_batch(streams)
    assert b["jobs"].size == 9000 and b["srcs"].size == 9000
    pcm, tails = graph_ref(oracle, streams, b, b["jobs"])
    want = np.concatenate([oracle.decode(os_, vol, [s], [lvl], 250) for os_, s, vol, lvl in streams])
    assert np.array_equal(pcm, want)            # (graph_ref is built from the oracle's primitives: the whole decode agrees)
    pcm.setflags(write=False)
    tails.setflags(write=False)
    return b, pcm, tails


def _live(ctx, b, lo, n, want_pcm, want_tails, what, first_prev=D.PREV_NONE, tails_in=None):
    """one live call over jobs [lo, lo + n) of `b`, held against those rows of the expected PCM (and tails); -> the tails it left"""
    srcs, jobs = _window(b, lo, n, first_prev)
    pcm, err, tails = ctx.decode_batch_live(b["blob"], srcs, jobs, tails_in=tails_in)
    _same(pcm, want_pcm[lo:lo + n], what + " pcm")
    assert not err.any(), what
    if want_tails is not None:
        _same(tails, want_tails[lo:lo + n], what + " tails")
    return tails


@pytest.mark.parametrize("zc", list(ZC))
def test_pinned_arenas_grow_past_their_first_size_and_serve_small_calls_after(dcs, long_lists, zc, monkeypatch):
    """the pinned arenas start at 1.5 MiB up and 2.25 MiB down (4 572 frames at 516 B): calls of 3, 6 000, 2, 9 000 and 5 frames
    on one context replace them twice (what they held is not kept) and go back to using their first bytes.  With the defaults
    6 000 frames are over both zero-copy thresholds, so the device arenas are made and grown too; then with copies always, and never."""
    if ZC[zc] is not None:
        monkeypatch.setenv("DCS_LIVE_ZC_UP_KB", ZC[zc][0])
        monkeypatch.setenv("DCS_LIVE_ZC_DOWN_FRAMES", ZC[zc][1])
    b, want, want_tails = long_lists
    ctx = dcs.Context(0)
    try:
        for lo, n in ((1250, 3), (0, 6000), (1750, 2), (0, 9000), (2250, 5)):
            _live(ctx, b, lo, n, want, want_tails, "%s: %d frames from %d" % (zc, n, lo))
    finally:
        ctx.close()


@pytest.mark.parametrize("order_seed", [0, 5])
def test_handoff_words_grow_twice_under_chains_that_cross_every_chunk(dcs, oracle, order_seed):
    """one frame per chunk, tails handed from chunk to chunk: calls of 300, 1 100, 2 100 and 300 chunks take the hand-off words
    from their first 1 024 chunks to 2 048 and 4 096 (cleared on growth, the epoch counting on), then a small call uses the large
    buffer; the chunks in plan order and in a seeded random one"""
    streams = [(os_for(ALL_FORMATS[k % 6], k), make_stream(ALL_FORMATS[k % 6], 300, seed=53000 + k, profile=k % 4), 250 - 5 * k, 0x64)
               for k in range(8)]
    b = D.build_stream_batch(streams)
    want = np.concatenate([oracle.decode(os_, vol, [s], [lvl], 300) for os_, s, vol, lvl in streams])
    calls = ((0, 300), (0, 1100), (0, 2100), (2100, 300))
    ctx = dcs.Context(0)
    try:
        ctx.set_frames_per_wave(4)
        ctx.set_frames_per_chunk(1)
        ctx.set_tail_handoff(True)
        ctx.set_test_hooks(chunk_order_seed=order_seed)
        for lo, n in calls:
            # (1 100 and 2 100 end inside a stream: its frames up to there are a chain of their own)
            _live(ctx, b, lo, n, want, None, "seed %d: %d frames from %d" % (order_seed, n, lo))
        # the chunk counts the case rests on: plan_chunks plans four frames to a chunk (it does not know the context's setting), so
        # a call has at least that many; with one frame per chunk -- the plan a batch of THIS context gets -- it has one per frame
        for (lo, n), floor in zip(calls, (75, 275, 525, 75)):
            srcs, jobs = _window(b, lo, n)
            assert D.plan_chunks(jobs, 4, srcs).shape[0] >= floor
            bt = ctx.batch(b["blob"], srcs, jobs)
            try:
                assert bt.num_chunks == n
            finally:
                bt.close()
        assert calls[1][1] + 1 > 1024 and calls[2][1] + 1 > 2048
    finally:
        ctx.close()


def _bad_jobs(jobs):
    """a job that is its own predecessor (validateBatch refuses it)"""
    bad = jobs.copy()
    bad["prev"][4] = 4
    return bad


@pytest.mark.parametrize("refused_first", [False, True])
def test_a_refused_call_leaves_the_live_state_usable(dcs, oracle, refused_first):
    """a call validateBatch refuses touches nothing: the next call continues from the tail the call before it left, and a context
    whose FIRST live call is refused decodes afterwards"""
    streams = [(os_for(f, 1), make_stream(f, 60, seed=54000 + f, profile=f % 4), 240, 0x60) for f in (D.FMT_94_T1_S3, D.FMT_93B_T1)]
    b = D.build_stream_batch(streams)
    want = np.concatenate([oracle.decode(os_, vol, [s], [lvl], 60) for os_, s, vol, lvl in streams])
    ctx = dcs.Context(0)
    try:
        tails = None
        if not refused_first:
            tails = _live(ctx, b, 60, 25, want, None, "before the refusal")
        srcs, jobs = _window(b, 0, 40)
        with pytest.raises(D.DcsError):
            ctx.decode_batch_live(b["blob"], srcs, _bad_jobs(jobs))
        if refused_first:
            _live(ctx, b, 60, 60, want, None, "first good call after a refused first call")
        else:
            _live(ctx, b, 85, 35, want, None, "continued after the refusal", first_prev=D.PREV_EXT | 0, tails_in=tails[-1:])
    finally:
        ctx.close()


def _mix_cases():
    meta = json.load(open(os.path.join(GOLD, "dcs_golden_hashes.json")))
    arrays = np.load(os.path.join(GOLD, "dcs_golden.npz"))
    out = []
    for case in meta["cases"]:
        if case["streams"] > 1:
            streams = [arrays["%s/stream%d" % (case["name"], c)].tobytes() for c in range(case["streams"])]
            out.append((case["name"], build_mix_batch(case["os"], case["volume"], streams, case["levels"], case["frames_out"]),
                        arrays[case["name"] + "/pcm"]))
    return sorted(out, key=lambda c: -len(c[1]["blob"]))


def test_what_one_blob_left_does_not_show_behind_a_shorter_ones_end(dcs):
    """the device blob is cleared as far as it was written when another blob takes its place: a named blob with 64 KiB of 0xFF
    appended (bytes no source points into), then a shorter case's blob without a name and under another name, then the first name
    again with less than was resident (the not-reuse branch) -- every PCM the golden one"""
    cases = _mix_cases()
    assert len(cases) >= 2
    (name_a, a, want_a), (name_b, b, want_b) = cases[0], cases[-1]
    assert len(b["blob"]) < len(a["blob"])
    ctx = dcs.Context(0)
    try:
        for what, m, blob, blob_id, want in (("long, extended, as 7", a, a["blob"] + b"\xff" * 65536, 7, want_a),
                                             ("short, unnamed", b, b["blob"], 0, want_b),
                                             ("short, as 8", b, b["blob"], 8, want_b),
                                             ("long, as 7 again", a, a["blob"], 7, want_a)):
            pcm, err, _ = ctx.decode_batch_live(blob, m["srcs"], m["jobs"], blob_id=blob_id)
            _same(pcm, want, "%s / %s: %s" % (name_a, name_b, what))
    finally:
        ctx.close()


def test_the_cache_is_not_involved(dcs, long_lists):
    """every arena of the live decoder grows (pinned and device, the hand-off words, the resident blob) and the context's cache
    holds what it held before; emptying the cache between two live calls changes nothing for the second"""
    b, want, want_tails = long_lists
    name, m, want_m = _mix_cases()[0]
    ctx = dcs.Context(0)
    try:
        before = ctx.cache_bytes()
        assert before[:2] == (0, 0)
        _live(ctx, b, 0, 3, want, want_tails, "3 frames")
        _live(ctx, b, 0, 6000, want, want_tails, "6 000 frames")
        pcm, err, _ = ctx.decode_batch_live(m["blob"], m["srcs"], m["jobs"], blob_id=3)
        _same(pcm, want_m, name)
        ctx.trim_cache()
        _live(ctx, b, 250, 9000 - 250, want, want_tails, "8 750 frames after trim_cache")
        _live(ctx, b, 500, 4, want, want_tails, "4 frames")
        assert ctx.cache_bytes() == before
        bt = ctx.batch(b["blob"], *_window(b, 0, 250))                      # what the cache does hold is a batch's buffers
        bt.close()
        held = ctx.cache_bytes()
        assert held[0] > 0
        _live(ctx, b, 0, 9000, want, want_tails, "9 000 frames next to a filled cache")
        assert ctx.cache_bytes() == held
    finally:
        ctx.close()


def test_index_inputs_stay_resident_and_are_replaced_whole(dcs):
    """dcs_index_streams_gpu keeps its inputs on the device for dcs_index_streams_gpu_time: eight streams, then three others (fewer
    and shorter: the buffers of the first call serve), the records the host walk's each time; timing without inputs is refused; the
    device packer's temporaries come and go on the same context"""
    def streams(first, n):
        return [(os_for(ALL_FORMATS[k % 6], k), make_stream(ALL_FORMATS[k % 6], 20 + 7 * k, seed=55000 + k, profile=k % 5), 255, 0x64)
                for k in range(first, first + n)]
    ctx = dcs.Context(0)
    try:
        with pytest.raises(D.DcsError, match="dcs_index_streams_gpu_time: no resident index inputs"):
            ctx.index_gpu_time(iters=2)
        for lst in (streams(0, 8), streams(8, 3)):
            got = ctx.index_streams_gpu(lst)
            assert len(got) == len(lst)
            for (os_, data, _, _), (idx, info) in zip(lst, got):
                want_idx, want_info = D.index_stream(os_, data)
                assert idx.tobytes() == want_idx.tobytes()
                assert bytes(info) == bytes(want_info)
        assert ctx.index_gpu_time(iters=2) > 0
        b = D.build_stream_batch(streams(8, 3), extra_frames=1)
        for fpw in (4, 8):
            dev = ctx.pack_chunks_device(b["blob"], b["srcs"], b["jobs"], fpw)
            assert np.array_equal(dev, D.pack_chunks(b["blob"], b["srcs"], b["jobs"], fpw))
    finally:
        ctx.close()
