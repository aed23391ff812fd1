"""The short pre-pass of the kernels of single-source even-deal batches (transform94x8<STEPS, true>; dcs_batch_filled_bands,
dcsPrepassShort) -- on a real MI355X.  A batch records the most header bands any of its sources fills tile words for, and the
transform leaves out the partners 128 - i that lie behind the last word such a frame can fill.  Lists of 12 to 24 streams of 16
frames as tests/test_gpu_sole_source_kernel.py builds them; PCM and error words equal the oracle's, and PCM, error words and kept
tails equal those of the even-deal kernel with the setting at 0 (the full pre-pass), at one and at two chunks per wavefront.
Nothing here is a tolerance."""
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
from dcsexplorer_amd import workloads
from oracle.dcs_oracle import fnv1a64
from test_gpu_sole_source_kernel import FPW, GOLD, decode, every_way, oracle_single, same, streams_of

pytestmark = pytest.mark.gpu
MID_STRADDLE = 0x200


def filled_bands(ctx, b, mids=None):
    """what a batch of the list records, with the even deal forced at 8 frames per wavefront -> (filled bands, takes the kernel)"""
    ctx.set_frames_per_wave(FPW)
    ctx.set_even_deal(1)
    try:
        bt = ctx.batch(b["blob"], b["srcs"], b["jobs"], mids=mids)
        try:
            return bt.filled_bands, bt.sole_source_kernel
        finally:
            bt.close()
    finally:
        ctx.set_frames_per_wave(0)
        ctx.set_even_deal(-1)


def rows_of(oracle, streams):
    """the oracle's frame buffers of the list, words 0..255 as int16 [frames, 256]"""
    rows = []
    for os_, s, _, _ in streams:
        n = (s[0] << 8) | s[1]
        rows.append(oracle.decompress(os_, s, 0x7FFF, n)[0][:, :256].astype(np.int16))
    return np.concatenate(rows)


@pytest.mark.parametrize("nbands", list(range(9, 17)))
def test_the_highest_band_at_full_scale(gpu_ctx, oracle, nbands):
    """9 .. 16 header bands, one list each (every count has its own number of short steps: 8, 7, ... 2, 0); one stream in four
    has the widest samples in every band (profile 4), so the word right in front of the first partner left out is as large as
    a word gets.  The boundary is exercised only if that word IS the row's last non-zero one: checked on the oracle's rows."""
    streams = streams_of(nbands, 97000 + 256 * nbands)
    zj, up_to = D.api.prepass_short(nbands)
    rows = rows_of(oracle, streams)
    last = np.array([np.flatnonzero(r)[-1] if r.any() else -1 for r in rows])
    assert last.max() == up_to, (nbands, last.max(), up_to)
    peak = int(np.abs(rows[:, up_to].astype(np.int32)).max())
    print("%d bands: %d short steps, last word %d, peak there %d, rows that reach it %d of %d"
          % (nbands, zj, up_to, peak, int((last == up_to).sum()), len(rows)))
    assert peak >= 0x2000                       # (a property of the inputs: a quarter of full scale at the least)
    b = D.build_stream_batch(streams)
    assert filled_bands(gpu_ctx, b) == (nbands, True)
    want, want_err = oracle_single(oracle, streams)
    _, err, _, _ = every_way(gpu_ctx, b, want, "%d bands" % nbands, want_err=want_err)
    assert not err.any()


def test_fewer_than_nine_bands_count_as_nine(gpu_ctx, oracle):
    """the field has three bits: 16 - 7 stands for every lower count, where all eight steps are short anyway"""
    streams = streams_of(5, 97900)
    b = D.build_stream_batch(streams)
    assert filled_bands(gpu_ctx, b) == (9, True) and D.api.prepass_short(5)[0] == D.api.prepass_short(9)[0] == 8
    want, want_err = oracle_single(oracle, streams)
    every_way(gpu_ctx, b, want, "5 bands", want_err=want_err)


def test_the_batch_maximum_decides(gpu_ctx, oracle):
    """12- and 16-band streams in one list: the batch records 16 and no step is short, for the 12-band frames either"""
    streams = streams_of(12, 98000, per_format=2) + streams_of(16, 98300, per_format=2)
    assert 12 <= len(streams) <= 24
    b = D.build_stream_batch(streams)
    assert filled_bands(gpu_ctx, b) == (16, True)
    want, want_err = oracle_single(oracle, streams)
    _, err, _, _ = every_way(gpu_ctx, b, want, "12 and 16 bands", want_err=want_err)
    assert not err.any()
    # ... and 12 with 14: three steps are short where the 12-band frames alone would have five
    streams = streams_of(12, 98600, per_format=2) + streams_of(14, 98900, per_format=2)
    b = D.build_stream_batch(streams)
    assert filled_bands(gpu_ctx, b) == (14, True)
    want, want_err = oracle_single(oracle, streams)
    every_way(gpu_ctx, b, want, "12 and 14 bands", want_err=want_err)


def test_a_second_source_keeps_the_full_pre_pass(gpu_ctx):
    """a 1994+ mix with the deal forced: further sources can write any cell, so the batch records nothing (16), runs the kernel
    with the rounds of further sources and its full pre-pass, and equals its committed reference PCM"""
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
            assert bt.even_deal and not bt.sole_source_kernel and bt.filled_bands == 16
            bt.run()
            pcm, _ = bt.download()
            bt.close()
            same(pcm, arrays[case["name"] + "/pcm"], "%s, %d chunks per wavefront" % (case["name"], cpw))
    finally:
        gpu_ctx.set_frames_per_wave(0)
        gpu_ctx.set_chunks_per_wave(0)
        gpu_ctx.set_even_deal(-1)


def test_records_that_start_a_lane_later_count_as_sixteen_bands(gpu_ctx):
    """caller-made mid records may name an output index beyond the band's middle (dcs_batch_create_mids bounds it by the next
    band's start).  In a frame of 13 bands the last lane starts with the second half of band 11 and goes on through band 12: started
    at word 176 instead of 168 it fills words up to 199, behind the frame's own last word 191 and inside the partners that four
    short steps would leave out (points 97 and up).  The batch records 16, and the kernel's PCM, error words and tails stay those
    of the kernel with the full pre-pass.  (No oracle: the records are not the stream's.)"""
    assert D.api.even_deal_lane(13, 7)[:2] == (21, 3)           # units 21 .. 23: band 11's second half, band 12's two
    streams = streams_of(13, 99000)
    b = D.build_stream_batch(streams)
    assert filled_bands(gpu_ctx, b, mids=b["mids"]) == (13, True)
    plain = every_way(gpu_ctx, b, None, "the library's own records", mids=b["mids"])
    # frames whose band 11 lies where sixteen-word bands put it -- it starts at word 160, its middle is 8 words on -- and has no
    # straddling code (a strided band without a code in front of it would have moved it down)
    first = 16 * (11 - 1)
    at = np.flatnonzero((b["mids"][:, 0] == 1) & ((b["mids"][:, 11] >> 16) & (0x1FF | MID_STRADDLE) == first + 8))
    assert at.size >= 8
    for shift in (8, 1):
        mids = b["mids"].copy()
        mids[at, 11] += shift << 16
        assert filled_bands(gpu_ctx, b, mids=mids) == (16, True)
        moved = every_way(gpu_ctx, b, None, "lanes that start %d words later" % shift, mids=mids)
        assert not np.array_equal(moved[0], plain[0])           # (the records are looked at: the PCM is another)


def test_forty_launches_of_one_batch(gpu_ctx, oracle):
    streams = streams_of(10, 99300)
    b = D.build_stream_batch(streams)
    want, want_err = oracle_single(oracle, streams)
    for cpw in (1, 2):
        often = decode(gpu_ctx, b, cpw, True, launches=40)
        same(often[0], want, "forty launches, %d chunks per wavefront" % cpw)
        same(often[1], want_err, "forty launches, error words")


def test_the_headline_workload_has_five_short_steps(gpu_ctx):
    """survey3_65536 as bench.py builds it, by the library's own selection: twelve bands at the most, so five of the eight steps
    are short; against the committed hashes"""
    gold = json.load(open(os.path.join(GOLD, "dcs_golden_hashes.json")))["workloads"]["survey3_65536"]["stream_hashes"]
    b = workloads.build("survey3_65536")
    bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
    try:
        assert bt.even_deal and bt.sole_source_kernel and bt.frames_per_wave == FPW
        assert bt.filled_bands == 12 and D.api.prepass_short(12)[0] == 5
        bt.run()
        pcm, err = bt.download()
    finally:
        bt.close()
    assert not err.any()
    first = b["first_job"]
    assert ["%016x" % fnv1a64(pcm[first[k]:first[k + 1]].tobytes()) for k in range(len(first) - 1)] == gold
