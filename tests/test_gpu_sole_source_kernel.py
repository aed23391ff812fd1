"""dcsDecodeKernel<8, CPW, true, true> -- the even-deal kernels of batches none of whose jobs has a second source, without the unpack
rounds of further sources, without code of the 1993 family, with one straight-line transform pass (dcs_ctx_set_sole_source_kernel,
dcs_batch_sole_source_kernel) -- on a real MI355X.  PCM and error words equal the oracle's (the committed reference PCM where
there is one), and PCM, error words and kept tails equal those of the even-deal kernel every other batch runs (the setting at 0)
on the same batch, at one and at two chunks per wavefront.  Lists of 12 to 24 streams of 16 to 40 frames (the damaged
streams, taken from tests/mids_cases.py, have three).  Nothing here is a tolerance."""
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
from dcsexplorer_amd import workloads
from oracle.dcs_oracle import fnv1a64
from util import make_stream, os_for
import mids_cases
from test_gpu_two_chunks import links_between_chunks, link_kinds, shuffled_index, ALL_KINDS

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FPW = 8
FORMATS_94 = [D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3]
SLOT_EMPTY = 0x80
# per stream of a list: the survey's code statistics; every code of the layout, the fixed-width sample codes 7 to 16 among them; four
# bands in ten without a code; the widest samples in every band
PROFILES = (5, 3, 2, 4)
VOLUMES = (255, 120, 40, 200)


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(np.atleast_2d(got) != np.atleast_2d(want))
        raise AssertionError("%s: %d values differ in %d rows; first at %s" % (what, len(bad), len(set(bad[:, 0])), bad[0]))


def oracle_single(oracle, streams, extra=0):
    """PCM and error words of streams each played alone: the oracle's decode, and its per-frame stop | fatal << 1 over the frames
    the index pass calls valid"""
    pcm, err = [], []
    for os_, s, vol, lvl in streams:
        n = ((s[0] << 8) | s[1]) + extra
        pcm.append(oracle.decode(os_, vol, [s], [lvl], n))
        _, info = D.index_stream(os_, s)
        e = np.zeros(n, dtype=np.uint32)
        e[:info.nValidFrames] = oracle.decompress(os_, s, 0x7FFF, info.nValidFrames)[3].astype(np.uint32)
        err.append(e)
    return np.concatenate(pcm), np.concatenate(err)


def streams_of(nbands, seed, n_frames=16, per_format=4, stride_from=None):
    """per_format streams of each 1994+ layout (Type 0, Type 1 sub-types 0 and 3): code statistics, volume and -- where the frame
    has the bands for it -- the first strided band (header bit 6) differ from stream to stream"""
    out = []
    for k in range(3 * per_format):
        fmt, j = FORMATS_94[k % 3], k // 3
        sf = stride_from if stride_from is not None else (16, max(nbands // 2, 1), 2, max(nbands - 1, 1))[j % 4]
        out.append((os_for(fmt, k), make_stream(fmt, n_frames, seed=seed + 16 * k, profile=PROFILES[j % 4], stride_from=sf, nbands=nbands),
                    VOLUMES[(j + k) % 4], 0x64 - 3 * j))
    return out


def decode(ctx, b, cpw, sole, jobs=None, tails_in=None, mids=None, launches=1, hooks=None):
    """a resident batch at 8 frames per wavefront with the even deal forced, every frame's tail kept; sole: the setting at its
    rule, else at 0 -> (pcm, err, tails, chunks)"""
    ctx.set_frames_per_wave(FPW)
    ctx.set_chunks_per_wave(cpw)
    ctx.set_even_deal(1)
    ctx.set_sole_source_kernel(-1 if sole else 0)
    ctx.set_batch_tails(True)
    if hooks is not None:
        ctx.set_test_hooks(chunk_order_seed=hooks, no_xcd_ranges=True)
    try:
        bt = ctx.batch(b["blob"], b["srcs"], b["jobs"] if jobs is None else jobs, tails_in, mids=mids)
        try:
            assert bt.frames_per_wave == FPW and bt.chunks_per_wave == cpw and bt.even_deal
            assert bt.sole_source_kernel == sole
            for _ in range(launches):
                bt.run()
            return bt.download(want_tails=True) + (bt.num_chunks,)
        finally:
            bt.close()
    finally:
        ctx.set_frames_per_wave(0)
        ctx.set_chunks_per_wave(0)
        ctx.set_even_deal(-1)
        ctx.set_sole_source_kernel(-1)
        ctx.set_batch_tails(False)
        ctx.set_test_hooks(0, False)


def every_way(ctx, b, want_pcm, what, want_err=None, **kw):
    """one and two chunks per wavefront, the kernels without further-source rounds against the others: PCM against `want_pcm`
    (and the error words against `want_err`), the three outputs of all four launches the same -> (pcm, err, tails, chunks)"""
    first = None
    for cpw in (1, 2):
        for sole in (False, True):
            got = decode(ctx, b, cpw, sole, **kw)
            where = "%s, %d chunks per wavefront, sole %d" % (what, cpw, sole)
            if want_pcm is not None:
                same(got[0], want_pcm, where + ": pcm")
            if want_err is not None:
                same(got[1], want_err, where + ": err")
            if first is None:
                first = got
            for a, c, name in zip(got, first, ("pcm", "err", "tails", "chunks")):
                same(np.asarray(a), np.asarray(c), where + ": " + name + " against the first way")
    return first


def test_the_setting_and_the_selection(gpu_ctx):
    """-1 | 0 only; a single-source 12-band list picks the kernel at one and at two chunks per wavefront, by the library's own rules
    for the deal as well; with the setting at 0, or without the even deal, it does not; the setting is read at every launch.  A
    multi-source 1994+ mix with the deal forced does not either, and equals its committed reference PCM."""
    L = gpu_ctx.L
    for bad in (-2, 1):
        assert L.dcs_ctx_set_sole_source_kernel(gpu_ctx.h, bad) == D.api.ERR_INVALID_ARG
    assert L.dcs_ctx_set_sole_source_kernel(None, 0) == D.api.ERR_INVALID_ARG
    assert L.dcs_batch_sole_source_kernel(None) == 0
    b = D.build_stream_batch(streams_of(12, 91000))
    assert (b["jobs"]["nSrc"] == 1).all()
    try:
        gpu_ctx.set_frames_per_wave(FPW)
        for cpw in (1, 2):
            gpu_ctx.set_chunks_per_wave(cpw)
            bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
            assert bt.even_deal and bt.sole_source_kernel and bt.chunks_per_wave == cpw
            gpu_ctx.set_sole_source_kernel(0)
            assert not bt.sole_source_kernel
            gpu_ctx.set_sole_source_kernel(-1)
            assert bt.sole_source_kernel
            bt.close()
        gpu_ctx.set_even_deal(0)
        bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
        assert not bt.even_deal and not bt.sole_source_kernel
        bt.close()
        gpu_ctx.set_even_deal(-1)
        gpu_ctx.set_frames_per_wave(4)
        bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
        assert not bt.sole_source_kernel
        bt.close()
    finally:
        gpu_ctx.set_frames_per_wave(0)
        gpu_ctx.set_chunks_per_wave(0)
        gpu_ctx.set_even_deal(-1)
        gpu_ctx.set_sole_source_kernel(-1)
    meta = json.load(open(os.path.join(GOLD, "dcs_golden_hashes.json")))
    arrays = np.load(os.path.join(GOLD, "dcs_golden.npz"))
    from mixer_ref import build_mix_batch
    case = next(c for c in meta["cases"] if c["streams"] > 1 and c["os"] in (D.OS94, D.OS95))
    streams = [arrays["%s/stream%d" % (case["name"], c)].tobytes() for c in range(case["streams"])]
    mb = build_mix_batch(case["os"], case["volume"], streams, case["levels"], case["frames_out"])
    by_frame, off = {}, 0
    for s in streams:
        off = (off + 3) & ~3
        idx, _, m = D.index_stream_mids(case["os"], s)
        for f in range(len(idx)):
            by_frame[(off, int(idx["bitOff"][f]))] = m[f]
        off += len(s) + 64
    mids = np.stack([by_frame[(int(sd["streamOff"]), int(sd["idx"]["bitOff"]))] for sd in mb["srcs"]])
    assert (mb["jobs"]["nSrc"] > 1).any()
    gpu_ctx.set_frames_per_wave(FPW)
    gpu_ctx.set_even_deal(1)
    try:
        for cpw in (1, 2):
            gpu_ctx.set_chunks_per_wave(cpw)
            bt = gpu_ctx.batch(mb["blob"], mb["srcs"], mb["jobs"], mids=mids)
            assert bt.even_deal and not bt.sole_source_kernel
            bt.run()
            pcm, _ = bt.download()
            bt.close()
            same(pcm, arrays[case["name"] + "/pcm"], "%s, %d chunks per wavefront" % (case["name"], cpw))
    finally:
        gpu_ctx.set_frames_per_wave(0)
        gpu_ctx.set_chunks_per_wave(0)
        gpu_ctx.set_even_deal(-1)


@pytest.mark.parametrize("nbands", list(range(1, 17)))
def test_every_coded_band_count(gpu_ctx, oracle, nbands):
    """1 .. 16 header bands with the deal forced (frames of 14 bands and more do not gain and run the fourth round), twelve
    streams of 16 frames: Type 0 and Type 1; strided bands; the fixed-width sample codes and bands without a code (profiles 3, 4
    and 2); four volumes, so that the volume shift is not zero everywhere"""
    streams = streams_of(nbands, 91100 + 256 * nbands)
    b = D.build_stream_batch(streams)
    assert len(set(b["jobs"]["volShift"].tolist())) > 1
    if nbands > 2:
        hdr = np.array([np.frombuffer(s, dtype=np.uint8)[2:2 + nbands] for _, s, _, _ in streams])
        assert (hdr & 0x40).any() and not (hdr & 0x40).all()
    want, want_err = oracle_single(oracle, streams)
    _, err, _, _ = every_way(gpu_ctx, b, want, "%d bands" % nbands, want_err=want_err)
    assert not err.any()


def test_silent_jobs_an_odd_number_of_chunks_and_padding_slots(gpu_ctx, oracle):
    """fourteen streams of 23 frames and a chain of five jobs without a source, which run no unpack round at all: padding slots,
    43 chunks (the last wavefront of the two-chunk kernel has no second one) and padding wavefronts in the last workgroup"""
    streams = streams_of(12, 92000, n_frames=23) + streams_of(9, 92500, n_frames=23)[:2]
    b = D.build_stream_batch(streams)
    silent = np.zeros(5, dtype=D.api.JOB_DTYPE)
    silent["volShift"] = 8
    silent["xform"] = D.XFORM_94
    silent["prev"] = D.PREV_NONE
    silent["prev"][1:] = len(b["jobs"]) + np.arange(4)
    jobs = np.concatenate([b["jobs"], silent])
    plan = D.plan_chunks(jobs, FPW, b["srcs"], handoff=True)
    assert plan.shape[0] % 2 == 1 and (-(-plan.shape[0] // 2)) % 4 != 0 and (plan["flags"] & SLOT_EMPTY).any()
    want, want_err = oracle_single(oracle, streams)
    want = np.concatenate([want, np.zeros((5, 240), dtype=np.int16)])
    want_err = np.concatenate([want_err, np.zeros(5, dtype=np.uint32)])
    _, err, _, chunks = every_way(gpu_ctx, b, want, "silent jobs", want_err=want_err, jobs=jobs)
    assert chunks == plan.shape[0] and not err.any()


def test_tails_across_the_halves_and_inside_a_pair(gpu_ctx, oracle):
    """twelve chains of 40 frames, five chunks each: tails cross from the first half of the launch to the second, stay on one side,
    and go from a wavefront's first chunk to its second; with the chunks in seeded random orders (the test hook) also backwards.
    The plan says which kinds occur, the test checks that every kind did."""
    streams = streams_of(12, 93000, n_frames=40)
    b = D.build_stream_batch(streams)
    plan = D.plan_chunks(b["jobs"], FPW, b["srcs"], handoff=True)
    n = plan.shape[0]
    links = links_between_chunks(b["jobs"], plan)
    want, want_err = oracle_single(oracle, streams)
    seen = link_kinds(links, n)
    pcm, err, tails, chunks = every_way(gpu_ctx, b, want, "plan order", want_err=want_err)
    assert chunks == n and not err.any()
    for seed in (3, 11, 29):
        at = shuffled_index(n, seed)
        seen |= link_kinds([(at[p], at[c]) for p, c in links], n)
        _, _, t, _ = every_way(gpu_ctx, b, want, "chunk order %d" % seed, want_err=want_err, hooks=seed)
        same(t, tails, "chunk order %d: tails" % seed)
    assert seen == ALL_KINDS, seen


def test_external_tails_in_and_kept_tails_out(gpu_ctx, oracle):
    """twelve streams of 26 frames decoded in two calls: the second call's chains start from the tails the first one kept
    (DCS_PREV_EXT), in frames of the launch's first and second half"""
    streams = streams_of(11, 94000, n_frames=26)
    b = D.build_stream_batch(streams)
    want, _ = oracle_single(oracle, streams)
    first = np.asarray(b["first_job"], dtype=np.int64)
    cut = 11
    _, _, tails_whole, _ = every_way(gpu_ctx, b, want, "whole")
    assert tails_whole.any()
    in_a = np.concatenate([np.arange(first[k], first[k] + cut) for k in range(len(streams))])
    in_b = np.concatenate([np.arange(first[k] + cut, first[k + 1]) for k in range(len(streams))])
    new_index = np.full(len(b["jobs"]), -1, dtype=np.int64)

    def part(rows, ext_row_of):
        jobs = b["jobs"][rows].copy()
        new_index[:] = -1
        new_index[rows] = np.arange(rows.size)
        for i, j in enumerate(rows):
            p = int(b["jobs"]["prev"][j])
            if p == D.PREV_NONE:
                continue
            jobs["prev"][i] = new_index[p] if new_index[p] >= 0 else (D.PREV_EXT | ext_row_of[p])
        return jobs

    ja = part(in_a, {})
    pa, _, ta, _ = every_way(gpu_ctx, b, want[in_a], "first call", jobs=ja)
    same(ta, tails_whole[in_a], "tails the first call kept")
    last_of_a = {int(first[k] + cut - 1): k for k in range(len(streams))}
    tails_in = np.stack([ta[np.flatnonzero(in_a == j)[0]] for j in sorted(last_of_a, key=last_of_a.get)])
    jb = part(in_b, last_of_a)
    assert ((jb["prev"] & D.PREV_EXT) != 0).sum() >= len(streams)
    _, _, tb, _ = every_way(gpu_ctx, b, want[in_b], "second call", jobs=jb, tails_in=tails_in)
    same(tb, tails_whole[in_b], "tails the second call kept")


def damaged_cases(oracle):
    """of the seeded damaged streams of tests/mids_cases.py (one flipped byte each, 1994+ layouts, three frames): those in which a
    frame stops at a two-zeros code with one sample left (stop without fatal: the kernel goes over the band again and takes its
    contribution back) and those with a band-type code that no codebook answers to (fatal), up to twelve of each"""
    overshoot, fatal = [], []
    for name, os_, s in mids_cases.cases():
        if "_flip" not in name:
            continue
        _, info = D.index_stream(os_, s)
        if info.nValidFrames == 0:
            continue
        stops = oracle.decompress(os_, s, 0x7FFF, info.nValidFrames)[3]
        if (stops & 2).any() and len(fatal) < 12:
            fatal.append((os_, s + bytes(1024), 255, 0x64))
        elif ((stops & 3) == 1).any() and len(overshoot) < 12:
            overshoot.append((os_, s + bytes(1024), 255, 0x64))
    return overshoot, fatal


def test_damaged_streams(gpu_ctx, oracle):
    """the two-zeros overshoot with its replay, and the fatal band-type code: the reference's error words and PCM"""
    overshoot, fatal = damaged_cases(oracle)
    assert len(overshoot) >= 4 and len(fatal) >= 4
    streams = overshoot + fatal
    assert 12 <= len(streams) <= 24
    b = D.build_stream_batch(streams, extra_frames=2)
    want, want_err = oracle_single(oracle, streams, extra=2)
    _, err, _, _ = every_way(gpu_ctx, b, want, "damaged", want_err=want_err)
    assert (err & D.FRAME_FATAL).any() and ((err & D.FRAME_STOP) != 0)[(err & D.FRAME_FATAL) == 0].any()


def test_forty_launches_of_one_batch(gpu_ctx, oracle):
    """the hand-off buffer is never cleared: its words carry the launch's epoch, and the fortieth launch finds the thirty-ninth's"""
    streams = streams_of(12, 95000, n_frames=24)
    b = D.build_stream_batch(streams)
    want, want_err = oracle_single(oracle, streams)
    for cpw in (1, 2):
        once = decode(gpu_ctx, b, cpw, True)
        often = decode(gpu_ctx, b, cpw, True, launches=40)
        for a, c, name in zip(often, once, ("pcm", "err", "tails")):
            same(a, c, "forty launches, %d chunks per wavefront: %s" % (cpw, name))
        same(often[0], want, "forty launches vs oracle")
        same(often[1], want_err, "forty launches, error words")


def test_the_headline_workload_takes_the_kernel(gpu_ctx):
    """survey3_65536 as bench.py builds it, by the library's own rules: the even deal, two chunks per wavefront and the kernel
    without further-source rounds; against the committed hashes"""
    gold = json.load(open(os.path.join(GOLD, "dcs_golden_hashes.json")))["workloads"]["survey3_65536"]["stream_hashes"]
    b = workloads.build("survey3_65536")
    bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
    try:
        assert bt.even_deal and bt.sole_source_kernel and bt.frames_per_wave == FPW
        bt.run()
        pcm, err = bt.download()
    finally:
        bt.close()
    assert not err.any()
    first = b["first_job"]
    assert ["%016x" % fnv1a64(pcm[first[k]:first[k + 1]].tobytes()) for k in range(len(first) - 1)] == gold
