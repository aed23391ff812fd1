"""The band plan of unpack94 (first source of a frame, 8 frames per wavefront: planBand94 in dcs_kernels.hip.h) on a real MI355X.
A chunk's 8 x 16 band set-ups are made once, two per lane, and read back as records by the lanes that start a band; further
sources of a frame and the kernels with 4 and 16 frames per wavefront keep the set-up inside the rounds.  So every case here
runs at 8 frames per wavefront with one and with two chunks per wavefront, and again at 4 and 16 frames per wavefront: PCM and
error words are the oracle's, sample for sample, and the same four times.  Nothing here is a tolerance."""
import numpy as np
import pytest

import dcsexplorer_amd as D
from util import make_stream, os_for, corrupt

pytestmark = pytest.mark.gpu
SLOT_HALO, SLOT_EMPTY = 0x01, 0x80
FORMATS_94 = (D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3)
# (frames per wavefront, chunks per wavefront): the plan in both of its kernels, then the two kernels without it
VARIANTS = ((8, 1), (8, 2), (4, 0), (16, 0))


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(np.atleast_2d(got) != np.atleast_2d(want))
        raise AssertionError("%s: %d values differ in %d rows; first at %s" % (what, len(bad), len(set(bad[:, 0])), bad[0]))


def decode_every_way(ctx, b, jobs=None, tails_in=None, handoff=True, what=""):
    """the batch through the four VARIANTS -> PCM, error words and tails of the first, the other three being equal to them"""
    jobs = b["jobs"] if jobs is None else jobs
    first = None
    try:
        ctx.set_tail_handoff(handoff)
        for fpw, cpw in VARIANTS:
            ctx.set_frames_per_wave(fpw)
            ctx.set_chunks_per_wave(cpw)
            got = ctx.decode_batch(b["blob"], b["srcs"], jobs, tails_in=tails_in, want_tails=True)
            if fpw == 8:
                # (a resident batch reports which kernel it launches: the forced settings hold)
                bt = ctx.batch(b["blob"], b["srcs"], jobs, tails_in)
                assert (bt.frames_per_wave, bt.chunks_per_wave) == (fpw, cpw)
                bt.close()
            if first is None:
                first = got
            for a, c, name in zip(got, first, ("pcm", "err", "tails")):
                same(a, c, "%s fpw %d cpw %d %s" % (what, fpw, cpw, name))
    finally:
        ctx.set_frames_per_wave(0)
        ctx.set_chunks_per_wave(0)
        ctx.set_tail_handoff(True)
    return first


def oracle_single(oracle, streams, extra=0):
    """PCM and error words of streams each played alone: the oracle's decode, and its per-frame stop | fatal << 1 over the
    frames the index pass calls valid (the frame that stops a stream is its last one with a source)"""
    pcm, err = [], []
    for os_, s, vol, lvl in streams:
        n = ((s[0] << 8) | s[1]) + extra
        pcm.append(oracle.decode(os_, vol, [s], [lvl], n))
        _, info = D.index_stream(os_, s)
        e = np.zeros(n, dtype=np.uint32)
        stops = oracle.decompress(os_, s, 0x7FFF, info.nValidFrames)[3]
        e[:info.nValidFrames] = stops.astype(np.uint32)
        err.append(e)
    return np.concatenate(pcm), np.concatenate(err)


def concat_batches(parts):
    """several batch descriptions (build_stream_batch, build_mix_batch) as one list: blobs back to back, indices moved on"""
    blob, srcs, jobs = bytearray(), [], []
    n_src = n_job = 0
    for b in parts:
        while len(blob) & 3:
            blob.append(0)
        s, j = b["srcs"].copy(), b["jobs"].copy()
        s["streamOff"] += len(blob)
        j["firstSrc"] += n_src
        linked = (j["prev"] != D.PREV_NONE) & ((j["prev"] & D.PREV_EXT) == 0)
        j["prev"][linked] += n_job
        blob += b["blob"]
        srcs.append(s); jobs.append(j)
        n_src += len(s); n_job += len(j)
    return dict(blob=bytes(blob), srcs=np.concatenate(srcs), jobs=np.concatenate(jobs))


# ---- one chunk, and a second one that is all but empty ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS_94)
def test_one_chunk_and_a_ninth_frame(gpu_ctx, oracle, fmt):
    """8 frames: one chunk, every slot planned.  9 frames: a second chunk of one frame and seven empty slots, whose plan lanes
    write records nobody reads"""
    for n_frames, chunks in ((8, 1), (9, 2)):
        streams = [(os_for(fmt), make_stream(fmt, n_frames, seed=88000 + 16 * fmt + n_frames, profile=n_frames % 4, stride_from=11), 255, 0x64)]
        b = D.build_stream_batch(streams)
        plan = D.plan_chunks(b["jobs"], 8, b["srcs"], handoff=True)
        assert plan.shape[0] == chunks
        assert int(((plan[-1]["flags"] & SLOT_EMPTY) != 0).sum()) == (0 if n_frames == 8 else 7)
        pcm, err, _ = decode_every_way(gpu_ctx, b, what="%d frames" % n_frames)
        want, want_err = oracle_single(oracle, streams)
        same(pcm, want, "%d frames vs oracle" % n_frames)
        same(err, want_err, "%d frames, error words" % n_frames)
        assert not err.any()


# ---- every kind of band --------------------------------------------------------------------------------------------------------
NBANDS = (1, 2, 3, 9, 12, 16)
STRIDE_FROM = (0, 3, 16)


def matrix_streams(fmt):
    """profiles 0..5 x band counts x first strided band, five frames each (chunks of eight then mix streams, band counts and
    strides slot by slot)"""
    out = []
    for profile in range(6):
        for nbands in NBANDS:
            for stride_from in STRIDE_FROM:
                seed = 88100 + ((fmt * 6 + profile) * 17 + nbands) * 17 + stride_from
                s = make_stream(fmt, 5, seed=seed, profile=profile, stride_from=stride_from, nbands=nbands)
                out.append((os_for(fmt, profile), s, [255, 220, 0x67, 255, 240, 200][profile], [0x64, 0x7F, 0x64, 0x20, 0x50, 0x70][profile]))
    return out


def band_kinds(streams):
    """what the matrix covers, from the index pass's records: strided bands 0 and 1 (counts 7 and 8 halve to 3 and 4), Type-1
    pre-adjust on bands 0 to 2, bands without a code, raw bands (Type 0: codes 7..16 are fixed-width samples)"""
    seen = set()
    for os_, s, _, _ in streams:
        idx, info = D.index_stream(os_, s)
        hdr = bytes(info.header)
        for r in idx:
            nb = int(r["nBands"])
            types = r["bandType"][:nb]
            for band in (0, 1):
                if band < nb and hdr[band] & 0x40 and types[band] != 0:
                    seen.add("strided band %d" % band)
            if info.format != D.FMT_94_T0 and r["preAdj"] & 0xFFF:
                seen.add("pre-adjust")
            if (types == 0).any():
                seen.add("band without a code")
            if info.format == D.FMT_94_T0 and (types >= 7).any():
                seen.add("raw band")
            if (np.asarray([hdr[k] & 0x40 for k in range(nb)]) != 0).any() and nb == 16 and types[15] != 0 and hdr[15] & 0x40:
                seen.add("strided band 15")
    return seen


@pytest.mark.parametrize("fmt", FORMATS_94)
def test_every_kind_of_band(gpu_ctx, oracle, fmt):
    streams = matrix_streams(fmt)
    want_kinds = {"strided band 0", "strided band 1", "band without a code", "strided band 15"}
    want_kinds |= {"raw band"} if fmt == D.FMT_94_T0 else {"pre-adjust"}
    assert band_kinds(streams) >= want_kinds, want_kinds - band_kinds(streams)
    b = D.build_stream_batch(streams, extra_frames=1)
    pcm, err, _ = decode_every_way(gpu_ctx, b, what="matrix")
    want, want_err = oracle_single(oracle, streams, extra=1)
    same(pcm, want, "matrix vs oracle")
    same(err, want_err, "matrix, error words")
    assert not err.any()


# ---- frames of several sources ----------------------------------------------------------------------------------------------------
def mix_cases():
    """(os, volume, streams, levels, frames): two and three sources that differ in format and in band count"""
    mk = lambda fmt, n, k, nbands, stride: make_stream(fmt, n, seed=88300 + k, profile=k % 4, stride_from=stride, nbands=nbands)
    return [(D.OS94, 255, [mk(D.FMT_94_T1_S3, 19, 0, 16, 16), mk(D.FMT_94_T0, 13, 1, 9, 3)], [0x64, 0x50], 20),
            (D.OS95, 230, [mk(D.FMT_94_T0, 11, 2, 12, 0), mk(D.FMT_94_T1_S0, 17, 3, 16, 12), mk(D.FMT_94_T1_S3, 9, 4, 3, 16)], [0x60, 0x64, 0x40], 18)]


def test_further_sources_keep_the_set_up_in_the_rounds(gpu_ctx, oracle):
    """the first source of a frame is planned, the others are not, and all go into one tile row"""
    from mixer_ref import build_mix_batch
    for k, (os_, vol, streams, levels, frames) in enumerate(mix_cases()):
        b = build_mix_batch(os_, vol, streams, levels, frames)
        fmts = {int(b["srcs"]["format"][int(j["firstSrc"]) + r]) for j in b["jobs"] for r in range(int(j["nSrc"]))}
        assert len(fmts) == len(streams) and int(b["jobs"]["nSrc"].max()) == len(streams)
        assert len({int(x) for x in b["srcs"]["idx"]["nBands"]}) == len(streams)
        pcm, err, _ = decode_every_way(gpu_ctx, b, what="mix %d" % k)
        same(pcm, oracle.decode(os_, vol, streams, levels, frames), "mix %d vs oracle" % k)
        assert not err.any()


def test_a_1993_frame_and_a_1994_frame_in_one_chunk(gpu_ctx, oracle):
    """a two-source 1994+ chain and a 1993 stream in one list: a chunk holds frames of both families, the 1993 frame's slot gets
    records nobody reads"""
    from mixer_ref import build_mix_batch
    os_, vol, streams, levels, frames = mix_cases()[0]
    frames = 11
    s93 = [(os_for(D.FMT_93_T0), make_stream(D.FMT_93_T0, 7, seed=88350), 255, 0x64),
           (os_for(D.FMT_93B_T1), make_stream(D.FMT_93B_T1, 6, seed=88351), 240, 0x60)]
    b = concat_batches([build_mix_batch(os_, vol, streams, levels, frames), D.build_stream_batch(s93)])
    plan = D.plan_chunks(b["jobs"], 8, b["srcs"], handoff=True)
    families = [{int(b["jobs"]["xform"][int(sl["job"])]) for sl in ch if not sl["flags"] & SLOT_EMPTY} for ch in plan]
    assert any(len(f) == 2 for f in families)
    pcm, err, _ = decode_every_way(gpu_ctx, b, what="both families")
    want = np.concatenate([oracle.decode(os_, vol, streams, levels, frames), oracle_single(oracle, s93)[0]])
    same(pcm, want, "both families vs oracle")
    assert not err.any()


# ---- damaged streams ---------------------------------------------------------------------------------------------------------------
# (format, seed of the stream, seed of the damage): chosen with error_paths() below on the CPU so that every path occurs
DAMAGED = [(D.FMT_94_T0, 0, 0), (D.FMT_94_T0, 1, 1), (D.FMT_94_T1_S0, 1, 0), (D.FMT_94_T1_S0, 0, 5), (D.FMT_94_T1_S3, 1, 0), (D.FMT_94_T1_S3, 0, 2)]


def damaged_streams():
    return [(os_for(fmt), corrupt(make_stream(fmt, 12, seed=88400 + k, profile=k % 4, stride_from=16 if k % 2 else 9), seed=500 + d, nflips=2) + bytes(1024), 255, 0x64)
            for fmt, k, d in DAMAGED]


def error_paths(oracle, streams):
    """which error paths of the 1994+ unpacker the streams take, from the oracle and the index pass's records alone:
      fatal      a band-type code that no codebook answers to (the frame's flags: stop and fatal);
      overshoot  a two-zeros code with one sample left (stop without fatal; 1994+ frames stop for nothing else,
                 dcs_tables.cpp rules the third cause out), after which the kernel goes over the band again;
      after      such a frame in which the band that stopped it is not the last: the bands behind it are still parsed and
                 contribute nothing.  The oracle zeroes the stopping band and everything behind it, so the first coded band
                 whose cells are all zero is at or before the stopping band; it counts only where at least two coded bands lie
                 behind that one and all of them are zero as well."""
    seen = set()
    for os_, s, _, _ in streams:
        idx, info = D.index_stream(os_, s)
        fb, _, _, stops = oracle.decompress(os_, s, 0x7FFF, info.nValidFrames)
        hdr = bytes(info.header)
        for f in range(info.nValidFrames):
            if stops[f] & 2:
                seen.add("fatal")
            elif stops[f] & 1:
                seen.add("overshoot")
                nb = int(idx[f]["nBands"])
                start = [1] + [int(idx[f]["split"][k]["state"]) & 0x1FF for k in range(nb - 1)]
                zeroed = []
                for band in range(nb):
                    if idx[f]["bandType"][band] == 0:
                        continue
                    count = (7 if band == 0 else 8 if band == 1 else 32 if band == 15 else 16)
                    inc = 2 if hdr[band] & 0x40 else 1
                    count //= inc
                    cells = fb[f][start[band]:start[band] + count * inc:inc]
                    zeroed.append(not cells.any())
                if True in zeroed:
                    at = zeroed.index(True)
                    if len(zeroed) - at >= 3 and all(zeroed[at:]):
                        seen.add("after")
    return seen


def test_damaged_streams_take_every_error_path(gpu_ctx, oracle):
    streams = damaged_streams()
    assert error_paths(oracle, streams) == {"fatal", "overshoot", "after"}
    b = D.build_stream_batch(streams, extra_frames=2)
    pcm, err, _ = decode_every_way(gpu_ctx, b, what="damaged")
    want, want_err = oracle_single(oracle, streams, extra=2)
    same(pcm, want, "damaged vs oracle")
    same(err, want_err, "damaged, error words")
    assert (err & D.FRAME_FATAL).any() and ((err & D.FRAME_STOP) != 0)[(err & D.FRAME_FATAL) == 0].any()


# ---- one chain across a chunk boundary: halo slots, tails in and out ------------------------------------------------------------
def test_one_chain_across_a_chunk_boundary(gpu_ctx, oracle):
    """a stream decoded in two calls, each longer than a chunk: the second call takes the first one's last tail from outside,
    inside a call the tail crosses the chunk boundary by the hand-off buffer and, with that off, by a halo slot (a frame
    decoded a second time for its tail only: planned like any other)"""
    fmt = D.FMT_94_T1_S3
    s = make_stream(fmt, 26, seed=88500, profile=1, stride_from=13)
    streams = [(os_for(fmt), s, 255, 0x64)]
    b = D.build_stream_batch(streams)
    want = oracle_single(oracle, streams)[0]
    halo_plan = D.plan_chunks(b["jobs"], 8, b["srcs"], handoff=False)
    assert ((halo_plan["flags"] & SLOT_HALO) != 0).any()
    cut = 11
    for handoff in (True, False):
        whole, _, tails_whole = decode_every_way(gpu_ctx, b, handoff=handoff, what="whole")
        same(whole, want, "whole chain vs oracle")
        ja = b["jobs"][:cut].copy()
        pa, _, ta = decode_every_way(gpu_ctx, b, ja, handoff=handoff, what="first call")
        same(ta, tails_whole[:cut], "tails out")
        jb = b["jobs"][cut:].copy()
        jb["prev"] = np.arange(jb.size, dtype=np.int64) - 1
        jb["prev"][0] = D.PREV_EXT | 0
        pb, _, tb = decode_every_way(gpu_ctx, b, jb, tails_in=ta[cut - 1:cut], handoff=handoff, what="second call")
        same(np.concatenate([pa, pb]), want, "two calls vs oracle")
        same(tb, tails_whole[cut:], "tails out of the second call")
