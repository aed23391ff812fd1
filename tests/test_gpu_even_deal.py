"""The even deal of 1994+ frames to their eight unpack lanes (dcs_batch_create_mids, dcs_ctx_set_even_deal) on a real MI355X:
PCM and error words equal the oracle's at both deals, each forced, at one and at two chunks per wavefront.  The lists are
two chunks of 8 frames per stream (16 frames), so that a tail crosses a chunk boundary in every one.  Nothing here is a
tolerance."""
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
from dcsexplorer_amd import workloads
from oracle.dcs_oracle import fnv1a64
from util import make_stream, os_for, corrupt

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FPW = 8
FORMATS_94 = [D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3]
SLOT_HALO, SLOT_EMPTY = 0x01, 0x80


def oracle_streams(oracle, streams, extra=0):
    return np.concatenate([oracle.decode(os_, vol, [s], [lvl], ((s[0] << 8) | s[1]) + extra) for os_, s, vol, lvl in streams])


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(np.atleast_2d(got) != np.atleast_2d(want))
        raise AssertionError("%s: %d values differ in %d rows; first at %s" % (what, len(bad), len(set(bad[:, 0])), bad[0]))


def run(ctx, b, deal, cpw, mids=None, want_even=None, handoff=True):
    """a resident batch at 8 frames per wavefront with the deal forced -> (pcm, err)"""
    ctx.set_frames_per_wave(FPW)
    ctx.set_chunks_per_wave(cpw)
    ctx.set_even_deal(deal)
    ctx.set_tail_handoff(handoff)
    try:
        bt = D.api.Batch(ctx, b["blob"], b["srcs"], b["jobs"], mids=mids)
        try:
            assert bt.frames_per_wave == FPW and bt.chunks_per_wave == cpw
            assert bt.even_deal == (bool(deal) if want_even is None else want_even)
            bt.run()
            return bt.download()
        finally:
            bt.close()
    finally:
        ctx.set_frames_per_wave(0)
        ctx.set_chunks_per_wave(0)
        ctx.set_even_deal(-1)
        ctx.set_tail_handoff(True)


def all_ways(ctx, b, want_pcm, what, mids=None, handoff=True):
    """both deals, one and two chunks per wavefront: all four against `want_pcm`; -> the error words"""
    err0 = None
    for deal in (0, 1):
        for cpw in (1, 2):
            pcm, err = run(ctx, b, deal, cpw, mids=mids, handoff=handoff)
            same(pcm, want_pcm, "%s, deal %d, %d chunks per wavefront: pcm" % (what, deal, cpw))
            if err0 is None:
                err0 = err
            same(err, err0, "%s, deal %d, %d chunks per wavefront: err" % (what, deal, cpw))
    return err0


def streams_of(nbands, seed, stride_from=16, profile=5, n_frames=16):
    return [(os_for(fmt, k), make_stream(fmt, n_frames, seed=seed + 16 * k, profile=profile, stride_from=stride_from, nbands=nbands),
             220 + k, 0x64) for k, fmt in enumerate(FORMATS_94)]


def test_the_setting_and_the_rule(gpu_ctx):
    """-1 | 0 | 1 only; by its own rule a batch takes the deal where a frame gains by it and only at 8 frames per wavefront,
    with mid records and nothing but 1994+ sources"""
    L = gpu_ctx.L
    for bad in (-2, 2):
        assert L.dcs_ctx_set_even_deal(gpu_ctx.h, bad) == D.api.ERR_INVALID_ARG
    assert L.dcs_ctx_set_even_deal(None, 1) == D.api.ERR_INVALID_ARG
    for nbands, want in ((12, True), (16, False), (14, False)):
        b = D.build_stream_batch(streams_of(nbands, 88000))
        for fpw in (4, 8, 16):
            gpu_ctx.set_frames_per_wave(fpw)
            try:
                bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
                assert bt.even_deal == (want and fpw == 8), (nbands, fpw)
                bt.close()
                bt = gpu_ctx.batch(b["blob"], np.asarray(b["srcs"]), b["jobs"])        # (no mid records)
                assert not bt.even_deal
                bt.close()
            finally:
                gpu_ctx.set_frames_per_wave(0)
    mixed = D.build_stream_batch(streams_of(12, 88100) + [(os_for(D.FMT_93_T0), make_stream(D.FMT_93_T0, 16, seed=88101), 255, 0x64)])
    run(gpu_ctx, mixed, 1, 1, want_even=False)


@pytest.mark.parametrize("nbands", list(range(1, 17)))
def test_every_coded_band_count(gpu_ctx, oracle, nbands):
    """Type 0 and Type 1 sub-types 0 and 3 with 1 .. 16 header bands, 16 frames each: two chunks per stream"""
    streams = streams_of(nbands, 88200 + 64 * nbands)
    b = D.build_stream_batch(streams)
    err = all_ways(gpu_ctx, b, oracle_streams(oracle, streams), "%d bands" % nbands)
    assert not err.any()


@pytest.mark.parametrize("nbands,stride_from", [(12, 6), (13, 2), (9, 3), (15, 8)])
def test_strided_bands(gpu_ctx, oracle, nbands, stride_from):
    """bands of half the samples at stride 2: their halves are 4 samples, two tile words apart"""
    streams = streams_of(nbands, 89300 + nbands, stride_from=stride_from, profile=1)
    b = D.build_stream_batch(streams)
    hdr = np.frombuffer(streams[0][1], dtype=np.uint8)[2:2 + nbands]
    assert (hdr[stride_from:] & 0x40).all() and not (hdr[:stride_from] & 0x40).any()
    err = all_ways(gpu_ctx, b, oracle_streams(oracle, streams), "strided from %d of %d" % (stride_from, nbands))
    assert not err.any()


def test_straddling_code_at_a_split(gpu_ctx, oracle):
    """a two-zeros code across the middle of a band at which a lane starts: the lane before it ends one sample later"""
    streams = streams_of(12, 89400, n_frames=16) + streams_of(11, 89500, n_frames=16) + streams_of(13, 89600, n_frames=16)
    b = D.build_stream_batch(streams)
    used = 0
    for k, src in enumerate(b["srcs"]):
        nb = int(src["idx"]["nBands"])
        for q in range(1, 8):
            first, count, _ = D.even_deal_lane(nb, q)
            band = first if first < 2 else 1 + first // 2
            if count and first >= 2 and (first & 1) and (int(b["srcs"].mids[k, band]) >> 16) & 0x200:
                used += 1
    assert used >= 8
    err = all_ways(gpu_ctx, b, oracle_streams(oracle, streams), "straddles")
    assert not err.any()


def test_frames_in_error_next_to_clean_ones(gpu_ctx, oracle):
    """bit-flipped payloads: a frame with an error flag is never split, its neighbours are"""
    streams = []
    for k in range(6):
        fmt = FORMATS_94[k % 3]
        s = corrupt(make_stream(fmt, 16, seed=89700 + k, profile=5, nbands=12), seed=400 + k, nflips=2)
        streams.append((os_for(fmt), s + bytes(1024), 255, 0x64))
    b = D.build_stream_batch(streams, extra_frames=2)
    flags = b["srcs"]["idx"]["flags"]
    assert (flags != 0).any() and (flags == 0).sum() > 16
    assert (b["srcs"].mids[flags != 0] == 0).all()
    err = all_ways(gpu_ctx, b, oracle_streams(oracle, streams, extra=2), "corrupted")
    assert err.any()


def test_halo_and_padding_slots(gpu_ctx, oracle):
    """13 frames per stream (padding slots in the last chunk) with the tails handed over, and with halo slots instead"""
    streams = streams_of(12, 89800, n_frames=13) + streams_of(10, 89850, n_frames=13)
    b = D.build_stream_batch(streams, extra_frames=1)
    want = oracle_streams(oracle, streams, extra=1)
    for handoff in (True, False):
        plan = D.plan_chunks(b["jobs"], FPW, b["srcs"], handoff=handoff)
        assert (plan["flags"] & SLOT_EMPTY).any()
        assert bool(((plan["flags"] & SLOT_HALO) != 0).any()) == (not handoff)
        err = all_ways(gpu_ctx, b, want, "handoff %d" % handoff, handoff=handoff)
        assert not err.any()


def test_a_multi_source_frame(gpu_ctx):
    """frames mixed from several 1994+ sources: the first source is dealt in units, the further ones in whole bands; against
    the committed reference PCM"""
    meta = json.load(open(os.path.join(GOLD, "dcs_golden_hashes.json")))
    arrays = np.load(os.path.join(GOLD, "dcs_golden.npz"))
    from mixer_ref import build_mix_batch
    n = 0
    for case in meta["cases"]:
        if case["streams"] == 1 or case["os"] not in (D.OS94, D.OS95):
            continue
        streams = [arrays["%s/stream%d" % (case["name"], c)].tobytes() for c in range(case["streams"])]
        b = build_mix_batch(case["os"], case["volume"], streams, case["levels"], case["frames_out"])
        # the mid records of the sources: by stream (in the order build_mix_batch lays them out) and frame
        by_frame, off = {}, 0
        for s in streams:
            off = (off + 3) & ~3
            idx, _, m = D.index_stream_mids(case["os"], s)
            for f in range(len(idx)):
                by_frame[(off, int(idx["bitOff"][f]))] = m[f]
            off += len(s) + 64
        mids = np.stack([by_frame[(int(sd["streamOff"]), int(sd["idx"]["bitOff"]))] for sd in b["srcs"]])
        assert (b["jobs"]["nSrc"] > 1).any()
        all_ways(gpu_ctx, b, arrays[case["name"] + "/pcm"], case["name"], mids=mids)
        n += 1
    assert n >= 1


def test_both_transform_families_in_one_chunk(gpu_ctx, oracle):
    """neighbouring frames alternate among the six layouts: such a batch has sources that are no 1994+ frames and keeps whole
    bands whatever the setting says; its 1994+ frames still decode next to the others"""
    b = workloads.build("mixed_16384", n_streams=12, n_frames=16)
    want = oracle_streams(oracle, b["streams"])[b["perm"]]
    for cpw in (1, 2):
        pcm, err = run(gpu_ctx, b, 1, cpw, want_even=False)
        same(pcm, want, "interleaved layouts, %d chunks per wavefront" % cpw)
        assert not err.any()


def test_jobs_of_the_other_transform_keep_whole_bands(gpu_ctx, oracle):
    """the rule wants every job on the 1994+ transform: a list whose sources are all 1994+ frames but which also has (silent)
    jobs of the 1993 transform keeps whole bands even when the deal is asked for, and decodes as before"""
    streams = streams_of(12, 89900)
    b = D.build_stream_batch(streams)
    silent = np.zeros(8, dtype=D.api.JOB_DTYPE)
    silent["volShift"] = 8
    silent["xform"] = D.XFORM_93
    silent["prev"] = D.PREV_NONE
    silent["prev"][1:] = len(b["jobs"]) + np.arange(7)
    b = dict(b, jobs=np.concatenate([b["jobs"], silent]))
    want = np.concatenate([oracle_streams(oracle, streams), np.zeros((8, 240), dtype=np.int16)])
    for cpw in (1, 2):
        pcm, err = run(gpu_ctx, b, 1, cpw, want_even=False)
        same(pcm, want, "silent 1993 jobs, %d chunks per wavefront" % cpw)
        assert not err.any()


def test_the_rule_wants_half_of_the_sources_to_gain(gpu_ctx):
    """one short stream among sixteen-band ones: the frames that do not gain would run a fourth round, the batch keeps whole bands"""
    few, full = streams_of(12, 90000), streams_of(16, 90010)
    for streams, want in ((few + full, True), (few + full + full, False)):
        b = D.build_stream_batch(streams)
        gpu_ctx.set_frames_per_wave(FPW)
        try:
            bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"], mids=b["mids"])
            assert bt.even_deal == want
            bt.close()
        finally:
            gpu_ctx.set_frames_per_wave(0)


def test_caller_made_mid_records_cannot_break_the_launch(gpu_ctx):
    """mid records come from the caller like index records: ones that do not lie inside their frame and band are refused before
    anything is launched (bits beyond the frame or before the band, an output index outside the row, before the band's start
    or behind the next band's); consistent ones that belong to other bytes -- the records AND mids of another stream -- decode to
    garbage inside the kernel's LDS"""
    os_ = os_for(D.FMT_94_T1_S3)
    a = make_stream(D.FMT_94_T1_S3, 24, seed=90101, profile=5, nbands=12)
    b_ = make_stream(D.FMT_94_T1_S3, 24, seed=90102, profile=3, nbands=12)
    batch = D.build_stream_batch([(os_, a, 255, 0x64), (os_, b_, 255, 0x64)])
    srcs, mids = np.asarray(batch["srcs"]).copy(), batch["mids"]
    gpu_ctx.set_frames_per_wave(FPW)
    gpu_ctx.set_even_deal(1)
    try:
        start = srcs["idx"]["split"]["state"][5, 3 - 1] & 0x1FF             # band 3 of frame 5 starts here
        nxt = srcs["idx"]["split"]["state"][5, 3] & 0x1FF
        for band, word in ((3, 60000 | (int(mids[5, 3]) & 0xFFFF0000)),       # bits beyond the frame
                           (3, 0 | (int(mids[5, 3]) & 0xFFFF0000)),           # ... before the band's start
                           (3, (int(mids[5, 3]) & 0xFFFF) | (0x1F0 << 16)),   # output index outside the row
                           (3, (int(mids[5, 3]) & 0xFFFF) | (0 << 16)),       # ... 0: before the band's start
                           (3, (int(mids[5, 3]) & 0xFFFF) | ((int(start) - 1) << 16)),
                           (3, (int(mids[5, 3]) & 0xFFFF) | ((int(nxt) + 1) << 16)),      # behind the next band's start
                           (11, (int(mids[5, 11]) & 0xFFFF) | (257 << 16))):  # the last band: behind the row
            bad = mids.copy()
            bad[5, band] = word
            with pytest.raises(D.DcsError):
                gpu_ctx.batch(batch["blob"], srcs, batch["jobs"], mids=bad)
        # the library's own pass, and so do the other stream's records with the other stream's mids
        n = 24
        swapped, smids = srcs.copy(), mids.copy()
        swapped["idx"][:n], swapped["idx"][n:] = srcs["idx"][n:].copy(), srcs["idx"][:n].copy()
        smids[:n], smids[n:] = mids[n:].copy(), mids[:n].copy()
        for cpw in (1, 2):
            gpu_ctx.set_chunks_per_wave(cpw)
            bt = gpu_ctx.batch(batch["blob"], swapped, batch["jobs"], mids=smids)
            assert bt.even_deal
            bt.run()
            pcm, err = bt.download()
            bt.close()
            assert pcm.shape == (48, 240)
    finally:
        gpu_ctx.set_frames_per_wave(0)
        gpu_ctx.set_even_deal(-1)
        gpu_ctx.set_chunks_per_wave(0)


@pytest.mark.parametrize("wl", ["survey3_65536", "dcs94_65536"])
def test_full_size_against_the_committed_hashes(gpu_ctx, wl):
    """the workloads as bench.py builds them, by the library's own rule: survey3_65536 (12 bands) takes the deal, dcs94_65536 (16) does not"""
    gold = json.load(open(os.path.join(GOLD, "dcs_golden_hashes.json")))["workloads"][wl]["stream_hashes"]
    b = workloads.build(wl)
    bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
    try:
        assert bt.even_deal == (wl == "survey3_65536") and bt.frames_per_wave == FPW
        bt.run()
        pcm, err = bt.download()
    finally:
        bt.close()
    assert not err.any()
    first = b["first_job"]
    assert ["%016x" % fnv1a64(pcm[first[k]:first[k + 1]].tobytes()) for k in range(len(first) - 1)] == gold
