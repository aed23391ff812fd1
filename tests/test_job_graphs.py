"""Job lists whose prev links form any graph (dcs_hip.h, DcsFrameJob.prev), on the host: the graph reference against the
oracle's own decode where the graph is a chain, and the chunk planner's invariants on seeded random graphs -- forks,
forward links, cycles, links between streams, lists without links."""
import numpy as np
import pytest

import dcsexplorer_amd as D
from graph_ref import graph_ref, rewire, fork, permute, ring
from util import ALL_FORMATS, FORMAT_NAMES, make_stream, os_for

HALO, EXT_TAIL, EXPORT, IMPORT, KEEP_TAIL, EMPTY = 0x01, 0x02, 0x04, 0x08, 0x10, 0x80


@pytest.mark.parametrize("extra", [0, 2], ids=["bare", "taper"])
@pytest.mark.parametrize("fmt", ALL_FORMATS, ids=[FORMAT_NAMES[f] for f in ALL_FORMATS])
def test_graph_reference_equals_oracle_decode_on_chains(oracle, fmt, extra):
    """on linear chains the composition of decompress and transform is the oracle's decode, taper frames and the first frame's
    own mixing multiplier included"""
    streams = [(os_for(fmt, v), make_stream(fmt, 23 + 11 * v, seed=41000 + 8 * fmt + v, profile=(fmt + v) % 4), 200 + 55 * v, 0x50 + fmt)
               for v in (0, 1)]
    b = D.build_stream_batch(streams, extra_frames=extra)
    pcm, tails = graph_ref(oracle, streams, b, b["jobs"])
    want = np.concatenate([oracle.decode(os_, vol, [s], [lvl], ((s[0] << 8) | s[1]) + extra) for os_, s, vol, lvl in streams])
    assert np.array_equal(pcm, want)
    # (a chain's tails: each frame's own samples 240..255, which the next frame's first samples overlap with)
    assert tails.any()


def check_plan(jobs, fpw, handoff, srcs, blob):
    """the planner's invariants on any graph; -> (imports, halos)"""
    plan = D.plan_chunks(jobs, fpw, srcs, handoff=handoff)
    n = jobs.size
    flat = plan.reshape(-1)
    real = flat[(flat["flags"] & (HALO | EMPTY)) == 0]
    assert np.array_equal(np.sort(real["job"]), np.arange(n)), "every job exactly once as a real slot"
    prev = jobs["prev"].astype(np.int64)
    link = (prev & D.PREV_EXT) == 0
    named = np.zeros(n, bool)
    named[prev[link]] = True
    home, last_live = {}, {}
    for c, chunk in enumerate(plan):
        for pos, sl in enumerate(chunk):
            if not (sl["flags"] & EMPTY):
                last_live[c] = pos
                if not (sl["flags"] & HALO):
                    home[int(sl["job"])] = (c, pos)
    pk = D.pack_chunks(blob, srcs, jobs, fpw) if handoff else None
    if pk is not None:
        assert pk.shape[0] == plan.shape[0]
    importers = {}              # (chunk, position) of an exporter -> jobs that import from it
    n_import = 0
    for c, chunk in enumerate(plan):
        pad = False
        for pos, sl in enumerate(chunk):
            fl = int(sl["flags"])
            if fl & EMPTY:
                pad = True
                continue
            assert not pad, "padding only at the end of a chunk"
            j = int(sl["job"])
            if pk is not None:
                words = pk[c, 80 * pos: 80 * pos + 16].view("<u4")
                assert int(words[0]) == j and (int(words[1]) >> 8) & 0xFF == fl
            if fl & HALO:
                assert sl["prevSlot"] == 0xFF and not (fl & (IMPORT | EXPORT))
                continue
            assert bool(fl & KEEP_TAIL) == (not named[j]), "the tail is kept where no frame of the batch names this one"
            p = int(prev[j])
            if not link[j]:
                assert sl["prevSlot"] == 0xFF and not (fl & IMPORT)
                assert bool(fl & EXT_TAIL) == (p != D.PREV_NONE)
            elif fl & IMPORT:
                n_import += 1
                assert handoff and sl["prevSlot"] == 0xFF
                pc, ppos = home[p]
                assert pc < c and last_live[pc] == ppos and (plan[pc][ppos]["flags"] & EXPORT)
                if pk is not None:
                    assert int(pk[c, 80 * pos + 12: 80 * pos + 16].view("<u4")[0]) == pc, "prevJob names the exporting chunk"
                importers.setdefault((pc, ppos), []).append(j)
            else:
                ps = int(sl["prevSlot"])
                assert ps < pos, "an in-chunk predecessor lies before its successor"
                assert int(chunk[ps]["job"]) == p and not (chunk[ps]["flags"] & EMPTY)
    for c, chunk in enumerate(plan):
        for pos, sl in enumerate(chunk):
            if (sl["flags"] & (EXPORT | EMPTY)) == EXPORT:
                got = importers.get((c, pos), [])
                assert len(got) == 1, "export row of chunk %d (job %d) has importers %s" % (c, int(sl["job"]), got)
                if pk is not None:
                    assert int(pk[c, 80 * pos + 60: 80 * pos + 64].view("<u4")[0]) == got[0], "the row's nextJob is its importer"
    if not handoff:
        assert n_import == 0 and not (plan["flags"] & EXPORT).any()
    return n_import, int(((flat["flags"] & (HALO | EMPTY)) == HALO).sum())


def _streams(fmts, seed, n=None):
    return [(os_for(f, k), make_stream(f, n or 30 + 7 * k, seed=seed + k, profile=k % 4), 255, 0x64) for k, f in enumerate(fmts)]


def _graphs(seed):
    """seeded graph cases: (name, blob, srcs, jobs)"""
    rng = np.random.default_rng(seed)
    one = D.build_stream_batch(_streams([D.FMT_94_T1_S3], 42000 + seed, n=20))
    four = D.build_stream_batch(_streams([D.FMT_94_T1_S3, D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3], 42100 + seed), extra_frames=2)
    both = D.build_stream_batch(_streams(ALL_FORMATS, 42200 + seed), extra_frames=1)
    out = []
    for name, b in (("one", one), ("four", four), ("both", both)):
        jobs = b["jobs"]
        n = jobs.size
        out.append((name + "-rewired", b, rewire(jobs, rng, 0.1)))
        out.append((name + "-rewired-much", b, rewire(jobs, rng, 0.4)))
        out.append((name + "-permuted", b, permute(jobs, rng)))
        out.append((name + "-rewired-permuted", b, permute(rewire(jobs, rng, 0.2), rng)))
        f0, f1 = int(b["first_job"][0]), int(b["first_job"][1])
        out.append((name + "-ring", b, ring(jobs, f0, f1 - 1)))
        out.append((name + "-ring-permuted", b, permute(ring(jobs, f0, f1 - 1), rng)))
        none = jobs.copy()
        none["prev"] = D.PREV_NONE
        out.append((name + "-unlinked", b, none))
        # forks of 2..4 successors around every chunk boundary of every frames-per-wave variant
        fj = jobs
        for p in range(3, min(n - 6, 64), 4):
            succ = [q for q in (p + 1, p + 2 + int(rng.integers(4)), p + 5 + int(rng.integers(20))) if q < n and jobs["xform"][q] == jobs["xform"][p]]
            if len(succ) >= 2:
                fj = fork(fj, p, succ[: 2 + int(rng.integers(2))])
        out.append((name + "-forks", b, fj))
    return out


@pytest.mark.parametrize("handoff", [True, False], ids=["handoff", "halo"])
@pytest.mark.parametrize("fpw", [4, 8, 16])
def test_planner_invariants_on_random_graphs(fpw, handoff):
    """any graph (dcs_hip.h): every job once, every link served -- through LDS from a slot before it, or through the hand-off row of
    the last frame of an earlier chunk, which meets exactly ONE importer, the job its nextJob names (the rendezvous has two sides:
    a second importer of a row would overwrite nextJob and never meet the producer) -- or by a halo re-decode"""
    seen_import = seen_halo = 0
    for seed in range(3):
        for name, b, jobs in _graphs(7919 * seed + fpw):
            try:
                imp, halos = check_plan(jobs, fpw, handoff, b["srcs"], b["blob"])
            except AssertionError as e:
                raise AssertionError("seed %d graph %s fpw %d: %s" % (seed, name, fpw, e)) from None
            seen_import += imp
            seen_halo += halos
    assert seen_halo > 0 and (seen_import > 0) == handoff
