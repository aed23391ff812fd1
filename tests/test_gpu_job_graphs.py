"""Job lists whose prev links form any graph, on a real MI355X, against graph_ref bit for bit (PCM and every frame's tail): forks
whose successors lie in the producer's chunk and in later ones, permuted job order (forward links), cycles, links between streams,
silent frames as producers and consumers, external tails shared by several jobs.  Through dcs_decode_batch, a resident batch and
the live decoder, at every frames-per-wave variant, with the tail hand-off on and off, one frame per chunk and the chunks in
seeded random orders.  Before every graph decode the same context decodes a list of as many jobs over other streams, so that a
row the kernel fails to write holds wrong samples rather than right ones left by an earlier call."""
import numpy as np
import pytest

import dcsexplorer_amd as D
from graph_ref import graph_ref, rewire, fork, permute, ring, external
from util import ALL_FORMATS, FORMAT_NAMES, make_stream, os_for

pytestmark = pytest.mark.gpu

LAYOUTS = ALL_FORMATS + ["both"]
LAYOUT_IDS = [FORMAT_NAMES[f] for f in ALL_FORMATS] + ["both-transforms"]
SETTINGS = ([dict(fpw=f, handoff=h) for f in (4, 8, 16) for h in (True, False)] + [dict(fpc=1)]
            + [dict(order_seed=s) for s in (0, 1, 7)])


def _streams(layout, seed):
    if layout == "both":
        return [(os_for(f, k), make_stream(f, 30 + 3 * k, seed=seed + k, profile=k % 4), 255 - 20 * k, 0x50 + 4 * k)
                for k, f in enumerate(ALL_FORMATS)]
    return [(os_for(layout, k), make_stream(layout, n, seed=seed + k, profile=(layout + k) % 4), 255 - 40 * k, 0x58 + 8 * k)
            for k, n in enumerate((37, 53))]


def _fork(b, rng):
    jobs = b["jobs"]
    n = jobs.size
    for p in (7, 15, 31, int(b["first_job"][1]) + 3, int(b["first_job"][1]) + 15):
        succ = [q for q in (p + 1, p + 2, p + 9, p + 20) if q < n and jobs["xform"][q] == jobs["xform"][p]]
        jobs = fork(jobs, p, succ[: 2 + int(rng.integers(3))] if len(succ) > 2 else succ)
    return jobs, None


def _permuted(b, rng):
    return permute(rewire(b["jobs"], rng, 0.1), rng), None


def _cycles(b, rng):
    jobs = b["jobs"]
    fj = b["first_job"]
    for k in range(len(fj) - 1):
        jobs = ring(jobs, int(fj[k]), int(fj[k + 1]) - 1)
    return jobs, None


def _cross(b, rng):
    return rewire(b["jobs"], rng, 0.25), None


def _silent(b, rng):
    """the taper frames (nSrc 0) feed frames of their own stream and of the next one, and take tails from the middle of a stream"""
    jobs = b["jobs"].copy()
    fj = [int(x) for x in b["first_job"]]
    ns = len(fj) - 1
    for k in range(ns):
        last, nxt = fj[k + 1] - 1, fj[(k + 1) % ns]
        assert jobs["nSrc"][last] == 0 and jobs["nSrc"][last - 1] == 0
        for q in (fj[k] + 5, nxt + 10):
            if jobs["xform"][q] == jobs["xform"][last]:
                jobs["prev"][q] = last
        jobs["prev"][last - 1] = fj[k] + 20
    return jobs, None


def _external(b, rng):
    return external(b["jobs"], rng, 3, 0.15)


FAMILIES = {"forks": _fork, "permuted": _permuted, "cycles": _cycles, "cross-stream": _cross, "silent": _silent, "external": _external}


def _apply(ctx, st):
    ctx.set_frames_per_wave(st.get("fpw", 0))
    ctx.set_tail_handoff(st.get("handoff", True))
    ctx.set_frames_per_chunk(st.get("fpc", 0))
    if "order_seed" in st:
        ctx.set_test_hooks(chunk_order_seed=st["order_seed"], no_xcd_ranges=True)


def _reset(ctx):
    ctx.set_frames_per_wave(0)
    ctx.set_tail_handoff(True)
    ctx.set_frames_per_chunk(0)
    ctx.set_test_hooks(0, False)
    ctx.set_batch_tails(False)


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        f, i = bad[0]
        raise AssertionError("%s: %d samples differ in %d rows; first at row %d sample %d: got %d want %d"
                             % (what, len(bad), len(set(bad[:, 0])), f, i, got[f, i], want[f, i]))


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_graph_decodes_equal_the_graph_reference(gpu_ctx, oracle, layout, family):
    seed = 43000 + 97 * LAYOUTS.index(layout) + 13 * list(FAMILIES).index(family)
    rng = np.random.default_rng(seed)
    streams = _streams(layout, seed)
    b = D.build_stream_batch(streams, extra_frames=2)
    jobs, tails_in = FAMILIES[family](b, rng)
    # the decoy: as many jobs, other streams (cached device buffers and the live decoder's arena are recycled)
    d = D.build_stream_batch(_streams(layout, seed + 5000), extra_frames=2)
    assert d["jobs"].size == jobs.size
    d_tails = np.full((3, 16), 1234, np.int16)
    want, want_tails = graph_ref(oracle, streams, b, jobs, tails_in)
    prev = jobs["prev"].astype(np.int64)
    named = np.zeros(jobs.size, bool)
    named[prev[(prev & D.PREV_EXT) == 0]] = True
    assert want_tails.any()

    blob, srcs = b["blob"], b["srcs"]
    for st in SETTINGS:
        what = "%s %s %s" % (layout if layout == "both" else FORMAT_NAMES[layout], family, st)
        _apply(gpu_ctx, st)
        try:
            gpu_ctx.decode_batch(d["blob"], d["srcs"], d["jobs"], want_tails=True)
            pcm, err, tails = gpu_ctx.decode_batch(blob, srcs, jobs, tails_in=tails_in, want_tails=True)
            _same(pcm, want, "decode_batch " + what)
            _same(tails, want_tails, "decode_batch tails " + what)
            assert not err.any(), what

            gpu_ctx.decode_batch_live(d["blob"], d["srcs"], d["jobs"], tails_in=d_tails)
            pcm, err, tails = gpu_ctx.decode_batch_live(blob, srcs, jobs, tails_in=tails_in)
            _same(pcm, want, "live " + what)
            _same(tails, want_tails, "live tails " + what)
            assert not err.any(), what

            # a resident batch, run twice: by default the tails of the frames no frame names, the other rows zero; then every row
            for all_tails in (False, True):
                gpu_ctx.set_batch_tails(all_tails)
                bt = gpu_ctx.batch(d["blob"], d["srcs"], d["jobs"])
                bt.run()
                bt.download(want_tails=True)
                bt.close()
                bt = gpu_ctx.batch(blob, srcs, jobs, tails_in=tails_in)
                bt.run()
                bt.run()
                pcm, err, tails = bt.download(want_tails=True)
                bt.close()
                _same(pcm, want, "resident %s %s" % (all_tails, what))
                assert not err.any(), what
                if all_tails:
                    _same(tails, want_tails, "resident tails " + what)
                else:
                    _same(tails[~named], want_tails[~named], "resident chain-end tails " + what)
                    assert not tails[named].any(), "resident: rows of named frames are zero " + what
        finally:
            _reset(gpu_ctx)

    for fpw in (4, 8, 16):
        got = gpu_ctx.pack_chunks_device(blob, srcs, jobs, fpw)
        assert np.array_equal(got, D.pack_chunks(blob, srcs, jobs, fpw)), "device packer fpw %d" % fpw


def test_bad_predecessors_are_refused_before_launch(gpu_ctx, oracle):
    """validateBatch: a job that is its own predecessor, a predecessor past the list, an external row past tailsIn or without
    tailsIn, a predecessor of the other transform -- DcsError from every entry point, and the context decodes on afterwards"""
    streams = _streams("both", 44000)
    b = D.build_stream_batch(streams)
    blob, srcs, jobs = b["blob"], b["srcs"], b["jobs"]
    n = jobs.size
    j = int(b["first_job"][3]) + 4                          # a job of the 1994+ transform
    assert jobs["xform"][j] == D.XFORM_94 and jobs["xform"][5] == D.XFORM_93
    tails2 = np.zeros((2, 16), np.int16)
    cases = [("self", j, None), ("past the list", n, None), ("past the list, far", 0x7FFFFFFE, None),
             ("external row past tailsIn", D.PREV_EXT | 2, tails2), ("external without tailsIn", D.PREV_EXT | 0, None),
             ("other transform", 5, None)]
    for name, p, tin in cases:
        bad = jobs.copy()
        bad["prev"][j] = p
        with pytest.raises(D.DcsError):
            gpu_ctx.decode_batch(blob, srcs, bad, tails_in=tin)
        with pytest.raises(D.DcsError):
            gpu_ctx.decode_batch_live(blob, srcs, bad, tails_in=tin)
        with pytest.raises(D.DcsError):
            gpu_ctx.batch(blob, srcs, bad, tails_in=tin)
    want = np.concatenate([oracle.decode(os_, vol, [s], [lvl], (s[0] << 8) | s[1]) for os_, s, vol, lvl in streams])
    pcm, err = gpu_ctx.decode_batch(blob, srcs, jobs)
    _same(pcm, want, "after the refusals")
    assert not err.any()
