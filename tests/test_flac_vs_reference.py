"""The FLAC reader's restatement and host index against the compiled libnyquist / libFLAC (oracle/_ref/dcs_flacref and its
sanitizer build, `make -C oracle flacref`) on the seeded files of tests/flac_fuzz_cases.py; no GPU.  The screen (a file is
kept where the checker loads it and the sanitizer build has nothing to say) must not be hollow: the conditions on the kept
set are asserted here, on the reference alone, and the tallies printed.  The damaged files are held to the relation
tests/test_gpu_flac_vs_reference.py states, for the part of it the host decides."""
import collections
import hashlib

import numpy as np
import pytest

import dcsexplorer_amd as D
import flac_fuzz_cases as Z
import flac_ref as R

pytestmark = pytest.mark.skipif(not Z.checker_available(), reason=Z.MISSING)


def same_bits(a, b):
    return len(a) == len(b) and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def loads():
    """the checker's verdict on every well-formed file; computed once, never changed"""
    return Z.check_load([c.data for c in Z.well_formed()])


@pytest.fixture(scope="module")
def damaged_loads():
    return Z.check_load([d.data for d in Z.damaged()])


def kept(load):
    return load.kind == "loaded" and not load.reports


def test_the_writer_restores_what_it_drew():
    """flac_ref on every well-formed file returns the integers the generator drew (cut to the stream's width)"""
    for c in Z.well_formed():
        st, x, d = R.integers(c.data)
        assert st == R.OK and np.array_equal(x, R.cut(c.ints, c.fmt[2])), c.name
        assert (d["rate"], d["channels"], d["bitDepth"]) == c.fmt, c.name


def test_the_screen_is_not_hollow(loads):
    cases = Z.well_formed()
    keep = [c for c, l in zip(cases, loads) if kept(l)]
    aside = [(c.name, l.kind, l.text, l.reports) for c, l in zip(cases, loads) if not kept(l)]
    classes = collections.Counter((c.fmt[2], c.fmt[1]) for c in keep)
    runs = collections.Counter(r for c in keep for r in c.runs)
    types = collections.Counter(t for c in keep for t in c.types)
    print("\nwell-formed: %d files, %d kept, %d set aside; %d reports of signed value shifts that GCC defines, not counted"
          % (len(cases), len(keep), len(aside), sum(l.value_shifts for l in loads)))
    print("set aside:", collections.Counter((k, tuple(r)) for _, k, _, r in aside))
    print("kept by (depth, channels):", dict(classes))
    print("kept by unary run class:", dict(runs))
    print("kept by subframe type:", dict(types))
    assert len(keep) >= 0.9 * len(cases)
    assert all(classes[b, c] >= 30 for b in (8, 16, 24) for c in (1, 2)), classes
    assert all(runs[r] >= 20 for r in Z.RUN_CLASSES), runs
    assert all(types[t] >= 20 for t in Z.TYPES), types
    # nothing the format allows makes the reference throw or crash
    assert all(k == "loaded" for _, k, _, _ in aside), aside


def test_restatement_equals_the_checker(loads):
    """flac_ref's floats are the checker's bits, on every kept file (and on the files set aside too, which is not relied on)"""
    for c, l in zip(Z.well_formed(), loads):
        if not kept(l):
            continue
        want = R.values(c.data)
        assert l.channels == c.fmt[1] and l.rate == c.fmt[0] and l.count == len(want), c.name
        assert l.sha256 == hashlib.sha256(np.asarray(want, "<f4").tobytes()).hexdigest(), c.name
        assert l.values is None or same_bits(l.values, want), c.name


def test_host_parse_and_index_accept_every_kept_file(loads):
    for c, l in zip(Z.well_formed(), loads):
        if not kept(l):
            continue
        st, want = R.parse(c.data)
        got = D.flac_parse(c.data)
        assert st == R.OK and got["status"] == 0, (c.name, got["reason"])
        for k in ("minBlockSize", "maxBlockSize", "rate", "channels", "bitDepth", "totalSamples", "nValues", "nFrames", "firstFrameOffset",
                  "sampleFormat"):
            assert got[k] == want[k], (c.name, k)
        ist, frames = D.flac_index(c.data)
        _, ref_frames = R.index(c.data)
        assert ist == 0 and len(frames) == len(ref_frames), c.name
        for f, r in zip(frames, ref_frames):
            assert all(int(f[k]) == r[k] for k in r), (c.name, r)


def test_damaged_files_on_the_host(damaged_loads):
    """checker, flac_ref and dcs_flac_parse / dcs_flac_index on every damaged file: the host index refuses exactly what flac_ref
    says it refuses, with that status and frame; nothing the checker throws on is accepted; what the checker loads and
    flac_ref refuses is refused under a named stricter clause; what both accept is equal"""
    tally = collections.Counter()
    codes = collections.Counter()
    for d, l in zip(Z.damaged(), damaged_loads):
        p = Z.predict(d.data)
        got = D.flac_parse(d.data)
        if p["where"] == "host":
            assert got["status"] == p["status"], (d.name, got["reason"], p)
            if p["frame"] is not None:
                assert got["reason"].startswith("frame %d:" % p["frame"]), (d.name, got["reason"], p)
            assert D.flac_index(d.data)[0] == p["status"], d.name
            tally["refused by the host index"] += 1
        else:
            assert got["status"] == 0, (d.name, got["reason"], p)
            ist, frames = D.flac_index(d.data)
            assert ist == 0 and len(frames) == got["nFrames"] == len(R.index(d.data)[1]), d.name
        if p["where"] == "device":
            codes[p["code"]] += 1
        if l.kind == "threw":
            assert p["status"] in (R.BAD_STREAM, R.INVALID_ARG), (d.name, l.text)
            tally["checker threw, refused"] += 1
        elif kept(l) and p["status"] == R.OK:
            assert same_bits(l.values, R.values(d.data)), d.name
            tally["accepted and equal"] += 1
        elif l.kind == "loaded" and p["status"] != R.OK:
            clause = Z.stricter_clause(p)
            assert clause is not None, (d.name, p)
            tally["stricter: " + clause] += 1
        else:
            tally["checker crashed or screen reported"] += 1
    print("\ndamaged: %d files" % len(Z.damaged()), dict(tally), "device codes:", dict(codes))
    assert all(codes[c] >= 5 for c in Z.CODES), codes
    assert tally["refused by the host index"] >= 20 and tally["accepted and equal"] >= 20, tally
