"""How the kernels of single-source even-deal batches (dcsDecodeKernel<8, CPW, true, true>) put their PCM into memory -- on a real
MI355X.  Whatever instructions carry the samples out, every emitted frame's 240 samples, the first sixteen of a frame whose tail
comes from another chunk (they belong to the rendezvous), the error words and the kept tails must be what they were, and nothing
may be written for padding slots, halo slots and frames without a slot.  Lists of 12 streams of 16 to 40 frames as
tests/test_gpu_sole_source_kernel.py builds them: PCM and error words equal the oracle's, and PCM, error words and kept tails equal
those of the even-deal kernel with the setting at 0, which keeps the 4-byte stores of every other kernel, at one and at two chunks
per wavefront.  Nothing here is a tolerance."""
import json

import numpy as np
import pytest

import dcsexplorer_amd as D
from dcsexplorer_amd import workloads
from oracle.dcs_oracle import fnv1a64
from test_gpu_sole_source_kernel import (FPW, GOLD, SLOT_EMPTY, damaged_cases, decode, every_way, oracle_single, same, streams_of)
from test_gpu_two_chunks import links_between_chunks, link_kinds, shuffled_index, ALL_KINDS

pytestmark = pytest.mark.gpu
SLOT_HALO, SLOT_EXPORT, SLOT_IMPORT = 0x01, 0x04, 0x08


@pytest.mark.parametrize("nbands", [1, 5, 12, 13, 16])
def test_band_counts_and_volume_shifts(gpu_ctx, oracle, nbands):
    """1, 5, 12, 13 and 16 header bands, twelve streams of 16 frames (two chunks per stream: every second chunk imports its first
    sixteen samples); volume shifts 0 and 3 in every list"""
    streams = streams_of(nbands, 101000 + 256 * nbands)
    assert len(streams) == 12
    b = D.build_stream_batch(streams)
    shifts = set(b["jobs"]["volShift"].tolist())
    assert {0, 3} <= shifts, shifts
    plan = D.plan_chunks(b["jobs"], FPW, b["srcs"], handoff=True)
    assert (plan["flags"] & SLOT_IMPORT).any() and (plan["flags"] & SLOT_EXPORT).any()
    want, want_err = oracle_single(oracle, streams)
    _, err, tails, _ = every_way(gpu_ctx, b, want, "%d bands" % nbands, want_err=want_err)
    assert not err.any() and tails.any()


def test_padding_slots_a_padding_wavefront_and_a_job_without_a_source(gpu_ctx, oracle):
    """twelve streams of 23 frames and a chain of five jobs without a source: padding slots in every stream's last chunk, an odd
    number of chunks and padding wavefronts in the last workgroup; the frames next to the padding keep every sample, and the
    silent jobs' frames are written as zeros over a buffer the launch before left full"""
    streams = streams_of(12, 102000, n_frames=23)
    b = D.build_stream_batch(streams)
    silent = np.zeros(5, dtype=D.api.JOB_DTYPE)
    silent["volShift"] = 3
    silent["xform"] = D.XFORM_94
    silent["prev"] = D.PREV_NONE
    silent["prev"][1:] = len(b["jobs"]) + np.arange(4)
    jobs = np.concatenate([b["jobs"], silent])
    plan = D.plan_chunks(jobs, FPW, b["srcs"], handoff=True)
    assert plan.shape[0] % 2 == 1 and (-(-plan.shape[0] // 2)) % 4 != 0 and (plan["flags"] & SLOT_EMPTY).any()
    want, want_err = oracle_single(oracle, streams)
    want = np.concatenate([want, np.zeros((5, 240), dtype=np.int16)])
    want_err = np.concatenate([want_err, np.zeros(5, dtype=np.uint32)])
    _, err, _, chunks = every_way(gpu_ctx, b, want, "padding", want_err=want_err, jobs=jobs)
    assert chunks == plan.shape[0] and not err.any()


def test_chains_across_chunks_in_every_order(gpu_ctx, oracle):
    """twelve chains of 40 frames, five chunks each, in plan order and in three seeded chunk orders: the importing frame's first
    sixteen samples are finished by whichever side of the rendezvous arrives second, and the wide stores of either side leave
    them alone"""
    streams = streams_of(12, 103000, n_frames=40)
    b = D.build_stream_batch(streams)
    plan = D.plan_chunks(b["jobs"], FPW, b["srcs"], handoff=True)
    n = plan.shape[0]
    links = links_between_chunks(b["jobs"], plan)
    want, want_err = oracle_single(oracle, streams)
    seen = link_kinds(links, n)
    _, err, tails, chunks = every_way(gpu_ctx, b, want, "plan order", want_err=want_err)
    assert chunks == n and not err.any()
    for seed in (5, 13, 31):
        at = shuffled_index(n, seed)
        seen |= link_kinds([(at[p], at[c]) for p, c in links], n)
        _, _, t, _ = every_way(gpu_ctx, b, want, "chunk order %d" % seed, want_err=want_err, hooks=seed)
        same(t, tails, "chunk order %d: tails" % seed)
    assert seen == ALL_KINDS, seen


def test_forty_launches_of_one_batch(gpu_ctx, oracle):
    """PCM, error words and tails after the fortieth launch are those after the first"""
    streams = streams_of(12, 104000, n_frames=24)
    b = D.build_stream_batch(streams)
    want, want_err = oracle_single(oracle, streams)
    for cpw in (1, 2):
        once = decode(gpu_ctx, b, cpw, True)
        often = decode(gpu_ctx, b, cpw, True, launches=40)
        for a, c, name in zip(often, once, ("pcm", "err", "tails")):
            same(a, c, "forty launches, %d chunks per wavefront: %s" % (cpw, name))
        same(often[0], want, "forty launches vs oracle")
        same(often[1], want_err, "forty launches, error words")


def test_halo_slots(gpu_ctx, oracle):
    """with the hand-off off a chain crosses a chunk boundary by a halo slot: a frame decoded for its tail only, whose PCM
    belongs to the chunk before -- nothing of its row may reach memory"""
    streams = streams_of(12, 105000, n_frames=19)
    b = D.build_stream_batch(streams)
    plan = D.plan_chunks(b["jobs"], FPW, b["srcs"], handoff=False)
    assert (plan["flags"] & SLOT_HALO).any() and (plan["flags"] & SLOT_EMPTY).any()
    want, want_err = oracle_single(oracle, streams)
    gpu_ctx.set_tail_handoff(False)
    try:
        _, err, _, chunks = every_way(gpu_ctx, b, want, "halo slots", want_err=want_err)
    finally:
        gpu_ctx.set_tail_handoff(True)
    assert chunks == plan.shape[0] and not err.any()


def test_external_tails_in_and_kept_tails_out(gpu_ctx, oracle):
    """twelve streams of 26 frames in two calls: the second call's chains start from the tails the first one kept"""
    streams = streams_of(13, 106000, n_frames=26)
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
    _, _, ta, _ = every_way(gpu_ctx, b, want[in_a], "first call", jobs=ja)
    same(ta, tails_whole[in_a], "tails the first call kept")
    last_of_a = {int(first[k] + cut - 1): k for k in range(len(streams))}
    tails_in = np.stack([ta[np.flatnonzero(in_a == j)[0]] for j in sorted(last_of_a, key=last_of_a.get)])
    jb = part(in_b, last_of_a)
    assert ((jb["prev"] & D.PREV_EXT) != 0).sum() >= len(streams)
    _, _, tb, _ = every_way(gpu_ctx, b, want[in_b], "second call", jobs=jb, tails_in=tails_in)
    same(tb, tails_whole[in_b], "tails the second call kept")


def test_damaged_streams(gpu_ctx, oracle):
    """the seeded single-byte corruptions that stop a frame: the reference's error words and PCM"""
    overshoot, fatal = damaged_cases(oracle)
    assert len(overshoot) >= 4 and len(fatal) >= 4
    streams = overshoot + fatal
    b = D.build_stream_batch(streams, extra_frames=2)
    want, want_err = oracle_single(oracle, streams, extra=2)
    _, err, _, _ = every_way(gpu_ctx, b, want, "damaged", want_err=want_err)
    assert (err & D.FRAME_FATAL).any() and ((err & D.FRAME_STOP) != 0)[(err & D.FRAME_FATAL) == 0].any()


def test_the_headline_workload(gpu_ctx):
    """survey3_65536 as bench.py builds it, by the library's own selection, against the committed hashes"""
    gold = json.load(open(GOLD + "/dcs_golden_hashes.json"))["workloads"]["survey3_65536"]["stream_hashes"]
    b = workloads.build("survey3_65536")
    bt = gpu_ctx.batch(b["blob"], b["srcs"], b["jobs"])
    try:
        assert bt.even_deal and bt.sole_source_kernel and bt.frames_per_wave == FPW and bt.chunks_per_wave == 2
        bt.run()
        pcm, err = bt.download()
    finally:
        bt.close()
    assert not err.any()
    first = b["first_job"]
    assert ["%016x" % fnv1a64(pcm[first[k]:first[k + 1]].tobytes()) for k in range(len(first) - 1)] == gold
