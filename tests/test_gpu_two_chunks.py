"""dcsDecodeKernel<8, 2>, two chunks per wavefront (dcs_ctx_set_chunks_per_wave), on a real MI355X: with the variant forced, PCM,
error words and tails equal the one-chunk kernel's bit for bit, and the oracle's or the committed reference hashes where there
are any.  Wavefront w of H = ceil(chunks / 2) decodes chunk w, then chunk w + H: the cases are cut so that the last wavefront
has no second chunk, that the last workgroup has padding wavefronts, that tails cross H in both directions and stay inside one
wavefront's pair, and that the second pass meets everything the first one does (further sources, the other transform family,
frames in error, tails in and out).  Nothing here is a tolerance."""
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
from dcsexplorer_amd import workloads
from oracle.dcs_oracle import fnv1a64
from util import ALL_FORMATS, FORMAT_NAMES, make_stream, os_for, corrupt

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FPW = 8
SLOT_HALO, SLOT_IMPORT, SLOT_EMPTY = 0x01, 0x08, 0x80


def oracle_streams(oracle, streams, extra=0):
    return np.concatenate([oracle.decode(os_, vol, [s], [lvl], ((s[0] << 8) | s[1]) + extra) for os_, s, vol, lvl in streams])


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(np.atleast_2d(got) != np.atleast_2d(want))
        raise AssertionError("%s: %d values differ in %d rows; first at %s" % (what, len(bad), len(set(bad[:, 0])), bad[0]))


class forced:
    """the context at 8 frames per wavefront and `cpw` chunks per wavefront, both back to the library's rules afterwards"""
    def __init__(self, ctx, cpw):
        self.ctx, self.cpw = ctx, cpw

    def __enter__(self):
        self.ctx.set_frames_per_wave(FPW)
        self.ctx.set_chunks_per_wave(self.cpw)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.set_frames_per_wave(0)
        self.ctx.set_chunks_per_wave(0)
        self.ctx.set_test_hooks(0, False)
        self.ctx.set_batch_tails(False)


def run_resident(ctx, cpw, b, jobs=None, tails_in=None, launches=1):
    """a resident batch at `cpw` chunks per wavefront -> (pcm, err, tails, chunks)"""
    jobs = b["jobs"] if jobs is None else jobs
    with forced(ctx, cpw):
        ctx.set_batch_tails(True)
        bt = ctx.batch(b["blob"], b["srcs"], jobs, tails_in)
        try:
            assert bt.frames_per_wave == FPW and bt.chunks_per_wave == cpw
            for _ in range(launches):
                bt.run()
            return bt.download(want_tails=True) + (bt.num_chunks,)
        finally:
            bt.close()


def both_ways(ctx, b, jobs=None, tails_in=None, what=""):
    """one and two chunks per wavefront, through a resident batch and through dcs_decode_batch: all four the same; -> the first"""
    jobs = b["jobs"] if jobs is None else jobs
    p1, e1, t1, n = run_resident(ctx, 1, b, jobs, tails_in)
    p2, e2, t2, n2 = run_resident(ctx, 2, b, jobs, tails_in)
    assert n == n2
    same(p2, p1, what + " pcm"); same(e2, e1, what + " err"); same(t2, t1, what + " tails")
    with forced(ctx, 2):
        p3, e3, t3 = ctx.decode_batch(b["blob"], b["srcs"], jobs, tails_in=tails_in, want_tails=True)
    same(p3, p1, what + " one-shot pcm"); same(e3, e1, what + " one-shot err"); same(t3, t1, what + " one-shot tails")
    return p1, e1, t1, n


def links_between_chunks(jobs, plan):
    """(producer chunk, consumer chunk) of every tail that crosses a chunk boundary in `plan` (dcs_plan_chunks2)"""
    chunk_of = {}
    for c in range(plan.shape[0]):
        for sl in plan[c]:
            if not sl["flags"] & (SLOT_EMPTY | SLOT_HALO):
                chunk_of[int(sl["job"])] = c
    out = []
    for c in range(plan.shape[0]):
        for sl in plan[c]:
            if sl["flags"] & SLOT_IMPORT and not sl["flags"] & SLOT_EMPTY:
                out.append((chunk_of[int(jobs["prev"][int(sl["job"])])], c))
    return out


def test_the_setting_and_the_rule(gpu_ctx):
    """0 | 1 | 2 only; forced values hold at any size for 8 frames per wavefront and never for 4 and 16; the rule picks two
    chunks for more than one and at most two generations of a batch that has the chip to itself"""
    L = gpu_ctx.L
    for bad in (-1, 3):
        assert L.dcs_ctx_set_chunks_per_wave(gpu_ctx.h, bad) == D.api.ERR_INVALID_ARG
    assert L.dcs_ctx_set_chunks_per_wave(None, 1) == D.api.ERR_INVALID_ARG
    small = D.build_stream_batch([(os_for(D.FMT_94_T1_S3), make_stream(D.FMT_94_T1_S3, 40, seed=77001), 255, 0x64)])
    try:
        for fpw, cpw, want in ((8, 0, 1), (8, 1, 1), (8, 2, 2), (4, 2, 1), (16, 2, 1)):
            gpu_ctx.set_frames_per_wave(fpw)
            gpu_ctx.set_chunks_per_wave(cpw)
            bt = gpu_ctx.batch(small["blob"], small["srcs"], small["jobs"])
            assert bt.chunks_per_wave == want, (fpw, cpw)
            gpu_ctx.set_chunks_per_wave(2 if fpw == 8 else 0)        # (read at every launch, not when the batch is made)
            assert bt.chunks_per_wave == (2 if fpw == 8 else 1)
            bt.close()
    finally:
        gpu_ctx.set_frames_per_wave(0)
        gpu_ctx.set_chunks_per_wave(0)
    places = 256 * 16
    for wl, want in (("survey3_65536", 2), ("dcs94_65536", 2), ("mixed_16384", 1), ("dcs93_4096", 1)):
        b = workloads.build(wl)
        bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
        in_rule = bt.frames_per_wave == 8 and places < bt.num_chunks <= 2 * places
        assert bt.chunks_per_wave == (2 if in_rule else 1) == want, wl
        gpu_ctx.set_concurrent_batches(True)
        try:
            shared = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
            assert shared.chunks_per_wave == 1, wl          # batches that share the chip keep the dynamic deal
            shared.close()
        finally:
            gpu_ctx.set_concurrent_batches(False)
        bt.close()


ODD_CASE_FRAMES = [5, 16, 20, 36, 57, 68, 100, 121]


def _odd_case(n_frames):
    fmt = D.FMT_94_T1_S3 if n_frames % 8 else D.FMT_93_T0
    streams = [(os_for(fmt), make_stream(fmt, n_frames, seed=77100 + n_frames, profile=n_frames % 4), 250, 0x66)]
    b = D.build_stream_batch(streams)
    return streams, b, D.plan_chunks(b["jobs"], FPW, b["srcs"], handoff=True).shape[0]


@pytest.mark.parametrize("n_frames", ODD_CASE_FRAMES)
def test_odd_chunk_counts_and_padding_wavefronts(gpu_ctx, oracle, n_frames):
    """1, 2, 3, 5, 8, 9, 13 and 16 chunks: a last wavefront without a second chunk, a last workgroup with one to three padding
    wavefronts, a launch that is one wavefront altogether"""
    streams, b, chunks = _odd_case(n_frames)
    pcm, err, _, n = both_ways(gpu_ctx, b, what="%d frames" % n_frames)
    assert n == chunks
    same(pcm, oracle_streams(oracle, streams), "%d frames vs oracle" % n_frames)
    assert not err.any()


def test_the_cases_above_cover_what_they_claim():
    """chunk counts of the parametrised test: odd ones, one chunk alone, and 0, 1, 2 and 3 padding wavefronts in the last workgroup"""
    counts = [_odd_case(n)[2] for n in ODD_CASE_FRAMES]
    halves = [-(-c // 2) for c in counts]
    assert sum(c % 2 for c in counts) >= 4 and 1 in counts and 2 in counts
    assert {h % 4 for h in halves} == {0, 1, 2, 3}


def shuffled_index(n_chunks, seed):
    """where dcs_ctx_set_test_hooks' chunk_order_seed puts chunk c of the plan (dcsShuffleChunks, dcs_plan.cpp)"""
    idx = list(range(n_chunks))
    x = seed
    for c in range(n_chunks - 1, 0, -1):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        k = (x >> 33) % (c + 1)
        idx[c], idx[k] = idx[k], idx[c]
    return idx


def link_kinds(links, n_chunks):
    H = -(-n_chunks // 2)
    kinds = set()
    for p, c in links:
        if c == p + H: kinds.add("pair, producer first")
        elif p == c + H: kinds.add("pair, consumer first")
        elif p < H <= c: kinds.add("first half to second")
        elif c < H <= p: kinds.add("second half to first")
        elif p < H: kinds.add("inside the first half")
        else: kinds.add("inside the second half")
    return kinds


ALL_KINDS = {"pair, producer first", "pair, consumer first", "first half to second", "second half to first",
             "inside the first half", "inside the second half"}


def test_tails_across_the_halves_and_inside_a_pair(gpu_ctx, oracle):
    """chains whose producer and consumer lie on either side of H, on one side, and in the two passes of ONE wavefront.  The
    planner puts a producer's chunk before its consumer's, so the plan as it is gives the forward kinds; the chunks in seeded
    random orders (the test hook, its permutation restated here) give the backward ones: consumer in the first half and producer
    in the second, and a wavefront whose FIRST chunk is the consumer.  The plan says which kinds occur, the test checks that
    every kind did."""
    forward, any_order = set(), set()
    cases = [([(D.FMT_94_T1_S3, 128)], (3, 11)), ([(D.FMT_93_T0, 120)], (5,)), ([(D.FMT_94_T0, 8), (D.FMT_94_T0, 8)], (1, 2, 3, 4)),
             ([(D.FMT_93B_T1, 12)], (1, 2, 3, 4)), ([(D.FMT_94_T1_S0, 70), (D.FMT_93A_T1, 24)], (9,))]
    for case, (parts, seeds) in enumerate(cases):
        streams = [(os_for(f, k), make_stream(f, n, seed=77200 + 10 * case + k, profile=(case + k) % 4), 255 - case, 0x64)
                   for k, (f, n) in enumerate(parts)]
        b = D.build_stream_batch(streams)
        jobs = b["jobs"]
        if len(parts) == 2 and parts[0] == parts[1]:
            jobs = jobs.copy()
            jobs["prev"][3] = int(b["first_job"][2]) - 1          # (a frame of the first stream takes the second stream's last tail)
        plan = D.plan_chunks(jobs, FPW, b["srcs"], handoff=True)
        n = plan.shape[0]
        links = links_between_chunks(jobs, plan)
        assert links
        forward |= link_kinds(links, n)
        want, _, want_tails, nch = both_ways(gpu_ctx, b, jobs, what="case %d" % case)
        assert nch == n
        if jobs is b["jobs"]:
            same(want, oracle_streams(oracle, streams), "case %d vs oracle" % case)
        for seed in seeds:
            at = shuffled_index(n, seed)
            any_order |= link_kinds([(at[p], at[c]) for p, c in links], n)
            with forced(gpu_ctx, 2):
                gpu_ctx.set_test_hooks(chunk_order_seed=seed, no_xcd_ranges=True)
                pcm, err, tails = gpu_ctx.decode_batch(b["blob"], b["srcs"], jobs, want_tails=True)
            same(pcm, want, "case %d, chunk order %d" % (case, seed))
            same(tails, want_tails, "case %d, chunk order %d, tails" % (case, seed))
            assert not err.any()
    assert forward == ALL_KINDS - {"pair, consumer first", "second half to first"}, forward
    assert any_order == ALL_KINDS, any_order


@pytest.mark.parametrize("seed", [1, 7, 1234])
def test_chunks_in_seeded_random_orders(gpu_ctx, oracle, seed):
    """every layout in one list, the chunks shuffled (the test hook): which wavefront and which pass a chunk falls to is arbitrary"""
    streams = [(os_for(f, f), make_stream(f, 45 + 13 * f, seed=77300 + f, profile=f % 3), 240, 0x62 + f) for f in ALL_FORMATS]
    b = D.build_stream_batch(streams, extra_frames=1)
    want = oracle_streams(oracle, streams, extra=1)
    for cpw in (1, 2):
        with forced(gpu_ctx, cpw):
            gpu_ctx.set_test_hooks(chunk_order_seed=seed, no_xcd_ranges=True)
            pcm, err, tails = gpu_ctx.decode_batch(b["blob"], b["srcs"], b["jobs"], want_tails=True)
        same(pcm, want, "cpw %d seed %d" % (cpw, seed))
        assert not err.any()
        if cpw == 1:
            t1 = tails
    same(tails, t1, "tails seed %d" % seed)


def test_tails_out_and_external_tails_in(gpu_ctx, oracle):
    """streaming use across the two-chunk kernel: a stream decoded in two calls, the second taking the first one's last tail
    (DCS_PREV_EXT) in a frame that the SECOND pass decodes as well as in one of the first pass; every frame's tail kept"""
    for fmt in (D.FMT_93_T0, D.FMT_94_T1_S3):
        s = make_stream(fmt, 90, seed=77400 + fmt)
        streams = [(os_for(fmt), s, 255, 0x64)]
        b = D.build_stream_batch(streams)
        want = oracle_streams(oracle, streams)
        for cut in (17, 43):
            _, _, tails_whole, _ = both_ways(gpu_ctx, b, what="whole")
            ja = b["jobs"][:cut].copy()
            pa, _, ta, _ = both_ways(gpu_ctx, b, ja, what="first call, cut %d" % cut)
            same(ta, tails_whole[:cut], "tails of the first call")
            # second call: its first frame takes the external tail -- and so does, as a second consumer of the same row, the frame
            # at 40, which lies in the launch's second half (its chain is then another: compared one against two chunks only)
            jb = b["jobs"][cut:].copy()
            jb["prev"] = np.arange(jb.size, dtype=np.int64) - 1
            jb["prev"][0] = D.PREV_EXT | 0
            pb, _, tb, _ = both_ways(gpu_ctx, b, jb, tails_in=ta[cut - 1:cut], what="second call, cut %d" % cut)
            same(np.concatenate([pa, pb]), want, "%s two calls, cut %d" % (FORMAT_NAMES[fmt], cut))
            same(tb, tails_whole[cut:], "tails of the second call")
            jb2 = jb.copy()
            jb2["prev"][40] = D.PREV_EXT | 0
            both_ways(gpu_ctx, b, jb2, tails_in=ta[cut - 1:cut], what="external tail into the second half")


def test_chain_end_tails_only(gpu_ctx):
    """DCS_SLOT_KEEP_TAIL as a resident batch sets it by default: the last frame of every chain, chain ends inside chunks of both passes"""
    streams = [(os_for(f), make_stream(f, n, seed=77500 + f), 255, 0x64)
               for f, n in ((D.FMT_94_T1_S3, 21), (D.FMT_93_T0, 9), (D.FMT_94_T0, 14), (D.FMT_93B_T1, 30), (D.FMT_94_T1_S0, 11))]
    b = D.build_stream_batch(streams)
    got = []
    for cpw in (1, 2):
        with forced(gpu_ctx, cpw):
            bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
            bt.run(); bt.run()
            got.append(bt.download(want_tails=True))
            bt.close()
    for a, c, what in zip(got[0], got[1], ("pcm", "err", "tails")):
        same(c, a, what)
    ends = np.asarray(b["first_job"][1:], dtype=np.int64) - 1
    rest = np.ones(len(b["jobs"]), bool); rest[ends] = False
    assert got[1][2][ends].any() and not got[1][2][rest].any()


def test_multichannel_frames_in_the_second_pass(gpu_ctx):
    """frames mixed from several sources: the second pass runs unpack rounds r > 0 (sources fetched from the blob, not the package);
    against the committed reference PCM"""
    meta = json.load(open(os.path.join(GOLD, "dcs_golden_hashes.json")))
    arrays = np.load(os.path.join(GOLD, "dcs_golden.npz"))
    from mixer_ref import build_mix_batch
    n = in_second_pass = 0
    for case in meta["cases"]:
        if case["streams"] == 1:
            continue
        streams = [arrays["%s/stream%d" % (case["name"], c)].tobytes() for c in range(case["streams"])]
        b = build_mix_batch(case["os"], case["volume"], streams, case["levels"], case["frames_out"])
        assert len(b["jobs"]) > FPW                     # (more than one chunk: there is a second pass)
        plan = D.plan_chunks(b["jobs"], FPW, b["srcs"], handoff=True)
        H = -(-plan.shape[0] // 2)
        second = plan[H:]["job"][(plan[H:]["flags"] & SLOT_EMPTY) == 0]
        in_second_pass += int((b["jobs"]["nSrc"][second] > 1).any())
        pcm, err, _, _ = both_ways(gpu_ctx, b, what=case["name"])
        same(pcm, arrays[case["name"] + "/pcm"], case["name"] + " vs reference")
        n += 1
    assert n >= 4 and in_second_pass >= 2


def test_both_transform_families_in_one_wavefront(gpu_ctx, oracle):
    """the lane constants are kept from the first pass while the family stays the same: lists in which a wavefront's two chunks
    want different families, in which one CHUNK mixes them (frames interleaved), and in which the family changes back and forth"""
    # (a) first half 1994+, second half 1993, and the other way round: the wavefronts change family between their passes
    for k, (fa, fb) in enumerate(((D.FMT_94_T1_S3, D.FMT_93_T0), (D.FMT_93B_T1, D.FMT_94_T0), (D.FMT_93A_T1, D.FMT_94_T1_S0))):
        streams = [(os_for(fa), make_stream(fa, 64, seed=77600 + k, profile=k), 255, 0x64),
                   (os_for(fb), make_stream(fb, 64, seed=77650 + k, profile=k + 1), 230, 0x70)]
        b = D.build_stream_batch(streams)
        plan = D.plan_chunks(b["jobs"], FPW, b["srcs"], handoff=True)
        H = -(-plan.shape[0] // 2)
        xf = b["jobs"]["xform"]
        changes = [xf[int(plan[w][0]["job"])] != xf[int(plan[w + H][-1]["job"])] for w in range(plan.shape[0] - H)
                   if not plan[w + H][-1]["flags"] & SLOT_EMPTY]
        assert sum(changes) >= 4
        pcm, err, _, _ = both_ways(gpu_ctx, b, what="families by halves %d" % k)
        same(pcm, oracle_streams(oracle, streams), "families by halves %d vs oracle" % k)
        assert not err.any()
    # (b) neighbouring frames alternate among the six layouts: chunks that mix both families, in both passes
    b = workloads.build("mixed_16384", n_streams=30, n_frames=50)
    plan = D.plan_chunks(b["jobs"], FPW, b["srcs"], handoff=True)
    mixed = [len({int(b["jobs"]["xform"][int(sl["job"])]) for sl in ch if not sl["flags"] & SLOT_EMPTY}) > 1 for ch in plan]
    H = -(-plan.shape[0] // 2)
    assert any(mixed[:H]) and any(mixed[H:])
    pcm, err, _, _ = both_ways(gpu_ctx, b, what="interleaved layouts")
    same(pcm, oracle_streams(oracle, b["streams"])[b["perm"]], "interleaved layouts vs oracle")
    assert not err.any()


def test_every_layout_of_the_reference_encoder(gpu_ctx, oracle):
    """the recordings of tests/golden/encoder_golden.npz, made by the reference's own encoder in the six layouts it can write
    (1994+ Type 0, Type 1 sub-types 0 and 3; OS93b Type 0 and 1; OS93a Type 0): lists of all of them through the two-chunk
    kernel, per-stream hashes and PCM as committed"""
    meta = json.load(open(os.path.join(GOLD, "encoder_golden.json")))
    arrays = np.load(os.path.join(GOLD, "encoder_golden.npz"))
    by_extra = {}
    for c in meta["cases"]:
        s = arrays[c["name"] + "/stream"].tobytes()
        by_extra.setdefault(c["frames_out"] - ((s[0] << 8) | s[1]), []).append((c, s))
    formats = set()
    for extra, cases in by_extra.items():
        streams = [(c["os"], s, c["volume"], c["levels"][0]) for c, s in cases]
        b = D.build_stream_batch(streams, extra_frames=extra)
        for k, (c, _) in enumerate(cases):
            formats.add((c["os"], int(b["srcs"]["format"][int(b["jobs"]["firstSrc"][b["first_job"][k]])])))
        pcm, err, _, n = both_ways(gpu_ctx, b, what="encoder recordings")
        assert n > 2 and not err.any()
        first = b["first_job"]
        for k, (c, s) in enumerate(cases):
            part = pcm[first[k]:first[k + 1]]
            assert "%016x" % oracle.fnv1a64(part) == c["pcm_fnv1a64"], c["name"]
            if c["name"] + "/pcm" in arrays:
                same(part, arrays[c["name"] + "/pcm"], c["name"])
    assert len(formats) == 6, formats


def test_frames_that_flag_errors(gpu_ctx, oracle):
    """bit-flipped payloads of every layout: zeroed bands, stops, silence afterwards and the error words, in both passes"""
    streams = []
    for k in range(12):                 # (the layouts in turn, so that both halves of the launch hold all of them)
        for fmt in ALL_FORMATS:
            s = corrupt(make_stream(fmt, 20, seed=77700 + fmt * 16 + k, profile=k % 4), seed=300 + k, nflips=3)
            streams.append((os_for(fmt), s + bytes(1024), 255, 0x64))
    b = D.build_stream_batch(streams, extra_frames=2)
    pcm, err, _, n = both_ways(gpu_ctx, b, what="corrupted")
    same(pcm, oracle_streams(oracle, streams, extra=2), "corrupted vs oracle")
    plan = D.plan_chunks(b["jobs"], FPW, b["srcs"], handoff=True)
    H = -(-n // 2)
    for part in (plan[:H], plan[H:]):
        jobs = part["job"][(part["flags"] & (SLOT_EMPTY | SLOT_HALO)) == 0]
        assert err[jobs].any()


@pytest.mark.parametrize("wl", ["survey3_65536", "dcs94_65536"])
def test_full_size_against_the_committed_hashes(gpu_ctx, wl):
    """8 192 chunks, two per wavefront by the library's own rule and by force, against the one-chunk kernel and
    tests/golden/rank_golden_hashes.json (rank 0 decodes the workload as it is)"""
    rank = json.load(open(os.path.join(GOLD, "rank_golden_hashes.json")))["workloads"][wl]
    gold = json.load(open(os.path.join(GOLD, "dcs_golden_hashes.json")))["workloads"][wl]["stream_hashes"]
    b = workloads.build(wl)
    assert len(b["first_job"]) - 1 == rank["streams_per_rank"]
    p1, e1, t1, n = run_resident(gpu_ctx, 1, b)
    assert n == 8192
    first = b["first_job"]
    for cpw in (2, 0):
        if cpw:
            p, e, t, _ = run_resident(gpu_ctx, cpw, b)
        else:
            bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
            assert bt.chunks_per_wave == 2              # the rule: more than one generation, at most two
            bt.run()
            p, e = bt.download()
            t = None
            bt.close()
        same(p, p1, "%s cpw %d pcm" % (wl, cpw)); same(e, e1, "%s cpw %d err" % (wl, cpw))
        if t is not None:
            same(t, t1, "%s cpw %d tails" % (wl, cpw))
        assert not e.any()
        got = ["%016x" % fnv1a64(p[first[k]:first[k + 1]].tobytes()) for k in range(len(first) - 1)]
        assert got == rank["rank_stream_hashes"][0] == gold, wl


def test_many_launches_of_one_batch(gpu_ctx, oracle):
    """the hand-off words carry the launch's epoch: a resident batch run forty times with two chunks per wavefront, then switched
    to one and back between launches, on buffers another batch has used before"""
    for rep in range(2):
        streams = [(os_for(f), make_stream(f, 90, seed=77800 + 7 * rep + f, profile=(f + rep) % 4), 255, 0x64)
                   for f in (D.FMT_93_T0, D.FMT_94_T1_S3, D.FMT_93B_T1)]
        b = D.build_stream_batch(streams)
        want = oracle_streams(oracle, streams)
        with forced(gpu_ctx, 2):
            bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
            try:
                for k in range(40):
                    if k >= 30:
                        gpu_ctx.set_chunks_per_wave(1 + k % 2)
                    bt.run()
                    if k in (0, 1, 29, 38, 39):
                        pcm, err = bt.download()[:2]
                        same(pcm, want, "launch %d" % k)
                        assert not err.any()
                bt.run_many(5)
                same(bt.download()[0], want, "run_many")
            finally:
                bt.close()


def test_pipeline_and_live_decoder_with_the_variant_forced(dcs, oracle):
    """forced, the variant also runs where the rule would not pick it: the live decoder's launches and a context of concurrent
    batches (chunks in XCD ranges, padding workgroups)"""
    ctx = dcs.Context(0)
    try:
        streams = [(os_for(f, f), make_stream(f, 60 + 9 * f, seed=77900 + f, profile=f % 4), 255, 0x64) for f in ALL_FORMATS]
        b = D.build_stream_batch(streams, extra_frames=2)
        want = oracle_streams(oracle, streams, extra=2)
        ctx.set_frames_per_wave(FPW)
        ctx.set_chunks_per_wave(2)
        pcm, err, _ = ctx.decode_batch_live(b["blob"], b["srcs"], b["jobs"])
        same(pcm, want, "live decoder"); assert not err.any()
        ctx.set_concurrent_batches(True)
        bt = ctx.batch(b["blob"], b["srcs"], b["jobs"])
        assert bt.chunks_per_wave == 2
        bt.run(); bt.run()
        pcm, err = bt.download()[:2]
        bt.close()
        same(pcm, want, "XCD ranges"); assert not err.any()
    finally:
        ctx.close()
