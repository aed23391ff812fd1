"""The GPU decoder against the reference's UNMODIFIED decoder (oracle/_ref/dcs_decref, `make -C oracle decref`) and against its
restatement, on the seeded cases of tests/dec_cases.py, on a real MI355X: re-headed synthetic streams, 1994+ streams written
from the decoder's side, damaged streams and mixes on one decoder.

Every list of dec_cases.lists() -- 24 to 48 single-stream cases, the classes shuffled together, damaged streams next to clean
ones -- is decoded through every route that picks different device code: 4, 8 and 16 frames per wavefront; at 8 both deals of
1994+ frames; with the even deal forced one and two chunks per wavefront, with and without the kernels of single-source
batches; the library's own choice; the index kernel against the host walk, record for record; the four pipeline modes.  PCM
and error words equal the restatement's on every case (these comparisons never skip), and the PCM equals the reference's own
on every case it defines (dec_cases.undefined; skipped where the binary is absent).  Nothing here is a tolerance."""
import numpy as np
import pytest

import dcsexplorer_amd as D
import dec_cases as C
from mixer_ref import build_mix_batch

pytestmark = pytest.mark.gpu
EXTRA = 2                       # frames pulled behind every stream of a list (a case's own extra_frames is 0 .. 2)
LISTS = C.lists()
MIXES = C.mixes()


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(np.atleast_2d(got) != np.atleast_2d(want))
        raise AssertionError("%s: %d values differ in %d rows; first at %s" % (what, len(bad), len(set(bad[:, 0])), bad[0]))


def streams_of(cases):
    return [(c.os, c.chans[0][1], c.volume, c.chans[0][0]) for c in cases]


_WANT = {}


def want_of(oracle, name, cases):
    """(PCM, error words, first row of each case) of a list, every stream played alone with EXTRA frames behind it: the
    restatement's decode, and its stop | fatal << 1 over the frames up to the first that has one"""
    if name not in _WANT:
        pcm, err, first = [], [], [0]
        for c in cases:
            s = c.chans[0][1]
            n = C.n_frames(s) + EXTRA
            pcm.append(oracle.decode(c.os, c.volume, [s], [c.chans[0][0]], n))
            stops = C.flags(oracle, c)[0]
            bad = np.flatnonzero(stops)
            e = np.zeros(n, dtype=np.uint32)
            if bad.size:
                e[bad[0]] = stops[bad[0]]
            err.append(e)
            first.append(first[-1] + n)
        _WANT[name] = (np.concatenate(pcm), np.concatenate(err), np.array(first))
        for a in _WANT[name]:
            a.setflags(write=False)
    return _WANT[name]


def run_batch(ctx, b, fpw=0, deal=-1, cpw=0, sole=-1, mids=None):
    """a resident batch at the given settings -> (pcm, err, what the batch says of itself)"""
    ctx.set_frames_per_wave(fpw)
    ctx.set_chunks_per_wave(cpw)
    ctx.set_even_deal(deal)
    ctx.set_sole_source_kernel(sole)
    try:
        bt = ctx.batch(b["blob"], b["srcs"], b["jobs"], mids=mids)
        try:
            said = dict(fpw=bt.frames_per_wave, even=bt.even_deal, sole=bt.sole_source_kernel, cpw=bt.chunks_per_wave)
            bt.run()
            return bt.download() + (said,)
        finally:
            bt.close()
    finally:
        ctx.set_frames_per_wave(0)
        ctx.set_chunks_per_wave(0)
        ctx.set_even_deal(-1)
        ctx.set_sole_source_kernel(-1)


# (name, settings, what the batch must say of itself; `only94` stands for "the list has 1994+ streams only")
ROUTES = [("the library's choice", dict(), dict()),
          ("4 frames per wavefront", dict(fpw=4), dict(fpw=4, even=False, sole=False)),
          ("16 frames per wavefront", dict(fpw=16), dict(fpw=16, even=False, sole=False)),
          ("8 frames, whole bands", dict(fpw=8, deal=0), dict(fpw=8, even=False, sole=False)),
          ("8 frames, even deal", dict(fpw=8, deal=1), dict(fpw=8, even="only94", sole="only94")),
          ("even deal, 1 chunk, every kernel", dict(fpw=8, deal=1, cpw=1, sole=0), dict(fpw=8, even="only94", sole=False, cpw=1)),
          ("even deal, 1 chunk, single-source", dict(fpw=8, deal=1, cpw=1, sole=-1), dict(fpw=8, even="only94", sole="only94", cpw=1)),
          ("even deal, 2 chunks, every kernel", dict(fpw=8, deal=1, cpw=2, sole=0), dict(fpw=8, even="only94", sole=False, cpw=2)),
          ("even deal, 2 chunks, single-source", dict(fpw=8, deal=1, cpw=2, sole=-1), dict(fpw=8, even="only94", sole="only94", cpw=2))]


@pytest.mark.parametrize("k", range(len(LISTS)), ids=[name for name, _, _ in LISTS])
def test_every_route_equals_the_restatement(gpu_ctx, oracle, k):
    """a list through every batch setting, dcs_decode_batch and dcs_decode_streams: PCM and error words"""
    name, only94, cases = LISTS[k]
    streams = streams_of(cases)
    want_pcm, want_err, first = want_of(oracle, name, cases)
    b = D.build_stream_batch(streams, extra_frames=EXTRA)
    assert np.array_equal(b["first_job"], first) and (b["jobs"]["nSrc"] <= 1).all()
    for route, settings, says in ROUTES:
        pcm, err, said = run_batch(gpu_ctx, b, **settings)
        for key, value in says.items():
            assert said[key] == (only94 if value == "only94" else value), (name, route, key, said)
        same(pcm, want_pcm, "%s, %s: pcm" % (name, route))
        same(err, want_err, "%s, %s: err" % (name, route))
    pcm, err = gpu_ctx.decode_batch(b["blob"], b["srcs"], b["jobs"])
    same(pcm, want_pcm, "%s, dcs_decode_batch: pcm" % name)
    same(err, want_err, "%s, dcs_decode_batch: err" % name)
    pcm, err, first_job = gpu_ctx.decode_streams(streams, extra_frames=EXTRA)
    assert np.array_equal(first_job, first)
    same(pcm, want_pcm, "%s, dcs_decode_streams: pcm" % name)
    same(err, want_err, "%s, dcs_decode_streams: err" % name)
    assert want_err.any() and (want_pcm != 0).any(axis=1).sum() > len(want_pcm) // 2       # (flagged frames, and mostly sound)


@pytest.mark.parametrize("k", range(len(LISTS)), ids=[name for name, _, _ in LISTS])
def test_the_index_kernel_equals_the_host_walk(gpu_ctx, k):
    """dcs_index_streams_gpu against dcs_index_streams: every record and every summary"""
    name, _, cases = LISTS[k]
    streams = streams_of(cases)
    host, dev = D.index_streams(streams), gpu_ctx.index_streams_gpu(streams)
    assert len(host) == len(dev) == len(cases)
    for c, (hr, hi), (dr, di) in zip(cases, host, dev):
        assert hr.tobytes() == dr.tobytes(), (name, c.name)
        for field in ("nFrames", "nValidFrames", "nBytes", "format", "hdrLen", "formatType", "formatSubType", "payloadBits"):
            assert getattr(hi, field) == getattr(di, field), (name, c.name, field)
        assert bytes(hi.header) == bytes(di.header), (name, c.name)


@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["host-index", "device-index", "device-index-and-pack", "device-index-plan-and-pack"])
def test_the_pipeline_modes(gpu_ctx, oracle, mode):
    """every list through a pipeline with the index walk, the packer and the planner on the host or on the device, three lists in flight"""
    pipe = gpu_ctx.pipeline(3, index_on_device=mode >= 1, pack_on_device=mode >= 2, plan_on_device=mode == 3)
    try:
        got = []
        for k, (name, _, cases) in enumerate(LISTS):
            pipe.submit(streams_of(cases), extra_frames=EXTRA)
            if k >= 2:
                got.append(tuple(a.copy() for a in pipe.collect()[:3]))
        while len(got) < len(LISTS):
            got.append(tuple(a.copy() for a in pipe.collect()[:3]))
    finally:
        pipe.close()
    for (name, _, cases), (pcm, err, first) in zip(LISTS, got):
        want_pcm, want_err, want_first = want_of(oracle, name, cases)
        assert np.array_equal(first, want_first), name
        same(pcm, want_pcm, "%s, pipeline mode %d: pcm" % (name, mode))
        same(err, want_err, "%s, pipeline mode %d: err" % (name, mode))


def mids_of(os_, streams, b):
    """the mid records of a mix's sources: by stream (in the order build_mix_batch lays them out) and frame"""
    by_frame, off = {}, 0
    for s in streams:
        off = (off + 3) & ~3
        idx, _, m = D.index_stream_mids(os_, s)
        for f in range(len(idx)):
            by_frame[(off, int(idx["bitOff"][f]))] = m[f]
        off += len(s) + 64
    return np.stack([by_frame[(int(sd["streamOff"]), int(sd["idx"]["bitOff"]))] for sd in b["srcs"]])


@pytest.mark.parametrize("k", range(0, len(MIXES), 4), ids=lambda k: "mixes%02d-%02d" % (k, k + 3))
def test_mixes_on_one_decoder(gpu_ctx, oracle, k):
    """2 to 8 streams of one OS version on the channels of one decoder: dcs_decode_batch at 4, 8 and 16 frames per wavefront
    and, 1994+, a batch with the even deal forced (the first source dealt in units, the others in whole bands)"""
    for c in MIXES[k:k + 4]:
        streams, levels = [s for _, s in c.chans], [l for l, _ in c.chans]
        want = C.oracle_pcm(oracle, c)
        b = build_mix_batch(c.os, c.volume, streams, levels, C.frames_out(c))
        assert (b["jobs"]["nSrc"] > 1).any()
        for fpw in (4, 8, 16):
            gpu_ctx.set_frames_per_wave(fpw)
            try:
                pcm, err = gpu_ctx.decode_batch(b["blob"], b["srcs"], b["jobs"])
            finally:
                gpu_ctx.set_frames_per_wave(0)
            same(pcm, want, "%s, %d frames per wavefront" % (c.name, fpw))
            assert not err.any(), c.name
        if C.is94(c):
            for cpw in (1, 2):
                pcm, err, said = run_batch(gpu_ctx, b, fpw=8, deal=1, cpw=cpw, mids=mids_of(c.os, streams, b))
                assert said["even"] and not said["sole"] and said["cpw"] == cpw, (c.name, said)
                same(pcm, want, "%s, even deal, %d chunks per wavefront" % (c.name, cpw))
                assert not err.any(), c.name


def test_the_reference_itself(gpu_ctx, oracle):
    """the PCM of dcs_decode_streams (lists) and dcs_decode_batch (mixes) against what the compiled reference decoder gives for
    every case it defines, a child process a case; the other routes equal these by the tests above"""
    if not C.checker_available():
        pytest.skip(C.MISSING)
    kept = aside = 0
    for name, _, cases in LISTS:
        pcm, _, first = gpu_ctx.decode_streams(streams_of(cases), extra_frames=EXTRA)
        for i, (c, ref) in enumerate(zip(cases, C.run_reference(cases))):
            if C.undefined(oracle, c):
                aside += 1
                continue
            assert ref.kind == "decoded", (c.name, ref.status)
            same(pcm[first[i]:first[i] + C.frames_out(c)], ref.pcm, "%s in %s against the reference" % (c.name, name))
            kept += 1
    for c, ref in zip(MIXES, C.run_reference(MIXES)):
        b = build_mix_batch(c.os, c.volume, [s for _, s in c.chans], [l for l, _ in c.chans], C.frames_out(c))
        pcm, _ = gpu_ctx.decode_batch(b["blob"], b["srcs"], b["jobs"])
        assert ref.kind == "decoded" and not C.undefined(oracle, c), c.name
        same(pcm, ref.pcm, "%s against the reference" % c.name)
        kept += 1
    print("\n%d cases against the reference's own PCM, %d set aside" % (kept, aside))
    assert kept >= 600


def test_frames_past_their_256_words(gpu_ctx, oracle):
    """OS93 Type 0 streams whose headers take a frame past its row (dec_cases.past_the_row: 8, 9, 15 and 16 bands strided)
    next to clean streams: the list is decoded, not refused, through every route, and what lies past word 255 is dropped"""
    cases = [C.past_the_row(n, seed=n) for n in (8, 9, 15, 16)]
    cases = [cases[0], C.reheaded()[3], cases[1], cases[2], C.reheaded()[50], cases[3]]
    streams = streams_of(cases)
    want_pcm, want_err, first = want_of(oracle, "past the row", cases)
    assert not want_err.any()
    b = D.build_stream_batch(streams, extra_frames=EXTRA)
    assert int((b["srcs"]["idx"]["split"]["state"] & 0x1FF).max()) == 256
    for route, settings, _ in ROUTES:
        pcm, err, _ = run_batch(gpu_ctx, b, **settings)
        same(pcm, want_pcm, "%s: pcm" % route)
        same(err, want_err, "%s: err" % route)
    for (hr, hi), (dr, di) in zip(D.index_streams(streams), gpu_ctx.index_streams_gpu(streams)):
        assert hr.tobytes() == dr.tobytes() and hi.nBytes == di.nBytes
    for mode in range(4):
        pipe = gpu_ctx.pipeline(2, index_on_device=mode >= 1, pack_on_device=mode >= 2, plan_on_device=mode == 3)
        try:
            pipe.submit(streams, extra_frames=EXTRA)
            pcm, err = (a.copy() for a in pipe.collect()[:2])
        finally:
            pipe.close()
        same(pcm, want_pcm, "pipeline mode %d: pcm" % mode)
        same(err, want_err, "pipeline mode %d: err" % mode)
    if C.checker_available():
        for i, (c, ref) in enumerate(zip(cases, C.run_reference(cases))):
            if not C.overruns(c, 512):
                same(pcm[first[i]:first[i] + C.frames_out(c)], ref.pcm, "%s against the reference" % c.name)
