"""Test helper: a plain reference for a job list whose prev links form ANY graph (forks, forward links, cycles, links
between streams, external tails shared by several jobs), built from the oracle's primitives alone (decompress and
transform, which test_oracle_vs_ref.py holds to the compiled reference), and the graph builders the tests and
tools/fuzz_parity.py share.

Each frame's 16-sample tail is samples 240..255 of its own transform (DCSDecoderNative.cpp:569-575, :810-812), whatever
tail came into it, so a job's PCM needs only its own spectrum and its predecessor's tail.  Covers single-source and
silent jobs; multi-source jobs keep their chain coverage (mixer_ref.py)."""
import numpy as np

import dcsexplorer_amd as D


def _source_map(streams, batch):
    """streamOff -> (stream index, first source index of the stream)"""
    first_job = batch["first_job"]
    srcs, jobs = batch["srcs"], batch["jobs"]
    out = {}
    for k in range(len(streams)):
        js = jobs[int(first_job[k]):int(first_job[k + 1])]
        js = js[js["nSrc"] > 0]
        if js.size:
            s0 = int(js["firstSrc"].min())
            out[int(srcs[s0]["streamOff"])] = (k, s0)
    return out


def graph_ref(oracle, streams, batch, jobs, tails_in=None):
    """streams: the (os, bytes, volume, level) list `batch` was built from (D.build_stream_batch); jobs: any job list over
    batch's sources with single-source or silent jobs.  -> (pcm [nJobs, 240] int16, tails [nJobs, 16] int16)"""
    smap = _source_map(streams, batch)
    srcs = batch["srcs"]
    n = jobs.size
    xform_os = {}                       # a silent job's transform: any stream's OS version of that transform
    for os_, _, _, _ in streams:
        xform_os.setdefault(D.XFORM_93 if os_ in (D.OS93A, D.OS93B) else D.XFORM_94, os_)
    cache = {}
    bufs, oses = [], []
    for j in range(n):
        jb = jobs[j]
        if int(jb["nSrc"]) == 0:
            bufs.append(np.zeros(512, np.uint16))
            oses.append(xform_os[int(jb["xform"])])
            continue
        assert int(jb["nSrc"]) == 1, "graph_ref covers single-source and silent jobs"
        sd = srcs[int(jb["firstSrc"])]
        k, s0 = smap[int(sd["streamOff"])]
        os_, data = streams[k][0], streams[k][1]
        mm = int(sd["mixMul"])
        if (k, mm) not in cache:
            nf = (data[0] << 8) | data[1]
            cache[(k, mm)] = oracle.decompress(os_, data, mm, nf)[0]
        bufs.append(cache[(k, mm)][int(jb["firstSrc"]) - s0])
        oses.append(os_)
    tails = np.zeros((n, 16), np.int16)
    for j in range(n):
        _, ov, _ = oracle.transform(oses[j], bufs[j], int(jobs[j]["volShift"]), np.zeros(16, np.uint16))
        tails[j] = ov.view(np.int16)
    pcm = np.zeros((n, 240), np.int16)
    for j in range(n):
        prev = int(jobs[j]["prev"])
        if prev == D.PREV_NONE:
            t = np.zeros(16, np.int16)
        elif prev & D.PREV_EXT:
            t = np.asarray(tails_in, np.int16)[prev & 0x7FFFFFFF]
        else:
            t = tails[prev]
        pcm[j] = oracle.transform(oses[j], bufs[j], int(jobs[j]["volShift"]), t.view(np.uint16))[0]
    return pcm, tails


# ---------------------------------------------------------------------------------------------- graph builders
# Each takes a job list (a copy is returned) and a numpy Generator.  Links always join jobs of one transform.

def rewire(jobs, rng, frac):
    """re-point a fraction of the links at random jobs of the same transform: forks, forward links, links between streams"""
    jobs = jobs.copy()
    n = jobs.size
    for j in rng.choice(n, size=max(1, int(frac * n)), replace=False):
        same = np.flatnonzero(jobs["xform"] == jobs["xform"][j])
        same = same[same != j]
        if same.size:
            jobs["prev"][j] = int(rng.choice(same))
    return jobs


def fork(jobs, producer, successors):
    """jobs `successors` all take `producer`'s tail"""
    jobs = jobs.copy()
    for s in successors:
        assert s != producer and jobs["xform"][s] == jobs["xform"][producer]
        jobs["prev"][s] = producer
    return jobs


def permute(jobs, rng):
    """the same graph with the jobs in a random order (links then point forward as well as back)"""
    n = jobs.size
    perm = rng.permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    out = jobs[perm].copy()
    link = (out["prev"] & D.PREV_EXT) == 0
    out["prev"][link] = inv[out["prev"][link]]
    return out


def ring(jobs, first, last):
    """close the chain first..last into a cycle: job `first` takes the tail of `last`"""
    jobs = jobs.copy()
    jobs["prev"][first] = last
    return jobs


def external(jobs, rng, n_tails, frac):
    """a fraction of the jobs take one of n_tails external tails (several jobs share a row); -> (jobs, tails_in) with seeded
    random tails that include the extremes -32768 and 32767"""
    jobs = jobs.copy()
    n = jobs.size
    for j in rng.choice(n, size=max(n_tails, int(frac * n)), replace=False):
        jobs["prev"][j] = D.PREV_EXT | int(rng.integers(n_tails))
    tails = rng.integers(-32768, 32768, size=(n_tails, 16)).astype(np.int16)
    tails[0, ::2] = 32767
    tails[0, 1::2] = -32768
    if n_tails > 1:
        tails[1, :8] = -32768
        tails[1, 8:] = 32767
    return jobs, tails
