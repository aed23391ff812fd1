"""The decoder's restatement (oracle/dcs_oracle.c) and the host index pass against the reference's UNMODIFIED decoder as a program
of its own (oracle/_ref/dcs_decref and dcs_decref_san, `make -C oracle decref`), on the seeded cases of tests/dec_cases.py: re-headed
synthetic streams (R), 1994+ streams written from the decoder's side (W), damaged ones (D) and mixes on one decoder (M).  No GPU.

The reference indexes its tables with whatever band-type code a damaged stream leaves, so it defines nothing for a case in which
the restatement raises a fatal flag, and nothing where an OS93 Type 0 header sends a frame's samples behind its frame buffer
(dec_cases.overruns; INTEGRATION.md "Damaged streams"); on every other case the two must agree on every sample, the reference must end
normally and its sanitizer build (-fsanitize=bounds,shift,float-cast-overflow) must have nothing to report but the two kinds of
shift dec_cases.reports() counts: `<<` on a negative value, which GCC defines and the reference's transforms do on every stream,
and the OS93a scale shifted by 32 or more, which the library takes modulo 32 as the reference's x86 build does.  The comparisons with the binaries
skip where they are absent; the conditions on the set and the index pass's check need the restatement only."""
import collections
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import dec_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_cases():
    return C.reheaded() + C.written() + C.damaged() + C.mixes()


@pytest.fixture(scope="module")
def runs(oracle):
    """{case name: (plain Ref, sanitizer Ref)}"""
    if not C.checker_available():
        pytest.skip(C.MISSING)
    cases = all_cases()
    return {c.name: pair for c, pair in zip(cases, zip(C.run_reference(cases), C.run_reference(cases, san=True)))}


def test_the_set_meets_its_conditions(oracle):
    """the corners the suite's other streams never reach, counted from the headers and from what the restatement says of every case"""
    R, W, Dm, M = C.reheaded(), C.written(), C.damaged(), C.mixes()
    assert (len(R), len(W), len(Dm), len(M)) == (238, 118, 360, 40)
    assert len({c.name for c in all_cases()}) == len(all_cases())
    for c in R + W:
        assert 3 <= C.n_frames(c.chans[0][1]) <= 40, c.name
    for c in M:
        assert 2 <= len(c.chans) <= 8 and len({C.n_frames(s) for _, s in c.chans}) > 1 and len({l for l, _ in c.chans}) > 1, c.name
    assert {len(c.chans) for c in M} == set(range(2, 9)) and {c.os for c in M} == {D.OS93A, D.OS93B, D.OS94, D.OS95}
    for vol in C.FORCED_VOLUMES:
        assert any(c.volume == vol for c in R) and any(c.volume == vol for c in W)
    for lvl in C.FORCED_LEVELS:
        assert any(c.chans[0][0] == lvl for c in R) and any(c.chans[0][0] == lvl for c in W)
    # R and W: no flag the recipe does not ask for
    for c in R + W:
        assert C.fatal(oracle, c) == ("fatal" in c.tags) and C.stopped(oracle, c) == ("stop" in c.tags), c.name
    assert sum("fatal" in c.tags for c in W) == 4 and sum("stop" in c.tags for c in W) == 10
    for c in M:
        assert not C.fatal(oracle, c) and not C.stopped(oracle, c), c.name
    # 1994+ scale codes, from the restatement's band-type codes
    stats = [x for c in R + W if C.is94(c) for x in C.band_stats(oracle, c)]
    over = sum(1 for typ, _, _, total in stats if typ and total >= 64)
    exp0 = sum(1 for _, _, _, total in stats if (total >> 2) & 15 == 0)
    exp15 = sum(1 for _, _, _, total in stats if (total >> 2) & 15 == 15)
    assert over >= 30 and exp0 >= 20 and exp15 >= 20
    assert {total & 63 for _, _, _, total in stats} == set(range(64)) and {h for _, _, h, _ in stats} == set(range(64))
    assert {(typ, total & 63) for typ, _, _, total in stats} == {(t, v) for t in (0, 1) for v in range(64)}
    facts = [C.header_facts(c) for c in R + W if C.is94(c)]
    assert {(typ, sub) for typ, sub, _, _ in facts} == {(t, s) for t in (0, 1) for s in range(4)}
    assert {(typ, nb) for typ, _, nb, _ in facts if typ == 0} >= {(0, nb) for nb in range(17)}
    assert {(typ, nb) for typ, _, nb, _ in facts if typ == 1} >= {(1, nb) for nb in range(17)}
    subsets = {strided for _, _, _, strided in facts if not C.is_suffix(strided)}
    assert len(subsets) >= 30
    # what the writer wrote: every entry of every codebook, the deltas at both ends, the fixed widths at their extremes
    assert C.W_LOG["entries"] == {(w, e) for w in range(1, 7) for e in C.BOOK_ENTRIES[w]}
    assert {-16, 14} <= C.W_LOG["deltas"]
    assert {(w, v) for w in range(7, 17) for v in (-(1 << (w - 1)), (1 << (w - 1)) - 1)} <= C.W_LOG["fixed"]
    # OS93 header exponents beyond the synthetic writer's 1 .. 8
    exps = set()
    for c in R:
        s = c.chans[0][1]
        if not C.is94(c) and not (c.os == D.OS93A and s[2] & 0x80):
            bands = next((k for k in range(16) if s[2 + k] & 0x7F == 0x7F), 16)
            exps |= {(s[2 + k] >> 2) & 15 for k in range(bands)}
    assert exps == set(range(16))
    # D: the share the reference does not define stays under the cap, and both kinds of flag are well represented
    n_fatal, n_stop = sum(C.fatal(oracle, c) for c in Dm), sum(C.stopped(oracle, c) for c in Dm)
    by = collections.Counter((next(iter(c.tags)), "fatal" if C.fatal(oracle, c) else "stop" if C.stopped(oracle, c) else "clean") for c in Dm)
    print("\nD: %d cases, %d fatal, %d stop without fatal; by mutation: %s" % (len(Dm), n_fatal, n_stop, sorted(by.items())))
    print("R + W: %d Type 1 bands with a scale sum of 64 or more, exponent 0 in %d bands, 15 in %d, %d stride subsets that are no suffix"
          % (over, exp0, exp15, len(subsets)))
    assert n_fatal <= 0.4 * len(Dm) and n_fatal >= 40 and n_stop >= 40
    hit = {m for m, _ in C.MUTATIONS}
    assert {next(iter(c.tags)) for c in Dm} == hit
    source = {c.name: c.chans[0][1] for c in R + W}
    assert sum(c.chans[0][1][2:18] != source[c.name.split("_of_")[1]][2:18] for c in Dm if "header_flips" in c.tags) >= 60
    # the lists of the GPU test: 24 to 48 cases, every single-stream case once, the classes mixed in each
    lists = C.lists()
    assert sorted(c.name for _, _, l in lists for c in l) == sorted(c.name for c in C.singles())
    for name, only94, l in lists:
        assert 24 <= len(l) <= 48 and {c.cls for c in l} == {"R", "W", "D"}, name
        assert all(C.is94(c) for c in l) == only94
        flagged = [bool(C.fatal(oracle, c) or C.stopped(oracle, c)) for c in l]
        assert any(a != b for a, b in zip(flagged, flagged[1:])), name          # (damaged streams next to clean ones)


def test_the_reference_agrees_wherever_it_defines_the_answer(oracle, runs):
    """every case without a fatal flag: the reference ends normally, its sanitizer build reports nothing and answers the same, the
    PCM equals the restatement's on every sample and GetStreamInfo agrees"""
    tally, shifts = collections.Counter(), collections.Counter()
    for c in all_cases():
        plain, san = runs[c.name]
        if C.undefined(oracle, c):
            tally[c.cls, "set aside (fatal)" if C.fatal(oracle, c) else "set aside (behind the frame buffer)"] += 1
            continue
        tally[c.cls, "stop without fatal" if C.stopped(oracle, c) else "clean"] += 1
        info_defined = not C.overruns(c, 256)              # (GetStreamInfo has 256 words where the decoder has 512)
        assert plain.kind == "decoded" and (plain.status == 0 or not info_defined), (c.name, plain.kind, plain.status)
        said, value, masked = C.reports(san)
        assert san.kind == "decoded" and not said, (c.name, san.kind, said)
        shifts["value"] += value != 0
        shifts["masked"] += masked != 0
        want = C.oracle_pcm(oracle, c)
        assert plain.pcm.shape == want.shape
        bad = np.argwhere(plain.pcm != want)
        assert bad.size == 0, "%s: %d samples differ, first at frame %d sample %d" % (c.name, len(bad), bad[0][0], bad[0][1])
        assert np.array_equal(san.pcm, want), c.name
        if info_defined:
            for (_, s), info in zip(c.chans, plain.infos):
                assert info == oracle.stream_info(c.os, s), c.name
        tally[c.cls, "... of these, GetStreamInfo behind its 256 words"] += not info_defined
    print("\nkept and set aside, per class: %s" % sorted(tally.items()))
    print("kept cases whose sanitizer run shifts a negative value left: %d; whose OS93a scale is shifted by 32 or more: %d" % (shifts["value"], shifts["masked"]))
    assert sum(n for (_, what), n in tally.items() if what in ("clean", "stop without fatal")) >= 580


def test_the_reference_fails_only_where_the_restatement_says_fatal(oracle, runs):
    """every case on which the reference crashes, or its sanitizer build crashes or reports (dec_cases.reports), is one of those set
    aside: the restatement's fatal flag, or an OS93 Type 0 header that reaches behind the frame buffer"""
    crashed = reported = differs = 0
    aside = [c for c in all_cases() if C.undefined(oracle, c)]
    for c in all_cases():
        plain, san = runs[c.name]
        said = C.reports(san)[0]
        bad = plain.kind == "crashed" or san.kind == "crashed" or bool(said)
        crashed += plain.kind == "crashed"
        reported += bool(said) or san.kind == "crashed"
        if C.undefined(oracle, c) and plain.kind == "decoded":
            differs += not np.array_equal(plain.pcm, C.oracle_pcm(oracle, c))
        assert not bad or C.undefined(oracle, c), (c.name, plain.kind, plain.status, san.kind, said)
    print("\nof %d cases set aside (%d with a fatal flag, %d behind the frame buffer): the reference crashes on %d, its sanitizer build "
          "crashes or reports on %d, and it ends with other PCM than the restatement on %d"
          % (len(aside), sum(C.fatal(oracle, c) for c in aside), sum(not C.fatal(oracle, c) for c in aside), crashed, reported, differs))


# what dcs_index_streams refuses outright (nFrames == 0 in the stream's summary), and the words of INTEGRATION.md that say so
REFUSALS = {"zero frames": "a zero-frame stream"}


def test_the_index_pass_against_the_restatement(oracle):
    """D.index_streams on every stream of every case: the frames it calls valid end with the first frame the restatement flags,
    their bit offsets are the restatement's, and so are their stop words"""
    streams = [(c.os, s) for c in all_cases() for _, s in c.chans]
    refused = collections.Counter()
    flagged = 0
    for (os_, s), (idx, info) in zip(streams, D.index_streams(streams)):
        if info.nFrames == 0:
            refused["zero frames" if C.n_frames(s) == 0 else "?"] += 1
            continue
        n = C.n_frames(s)
        _, bit_offs, _, stops = oracle.decompress(os_, s, 0x7FFF, n)
        first_bad = next((f for f in range(n) if stops[f]), None)
        valid = n if first_bad is None else first_bad + 1
        flagged += first_bad is not None
        assert (info.nFrames, info.nValidFrames, len(idx)) == (n, valid, valid)
        assert np.array_equal(idx["bitOff"], bit_offs[:valid].astype(np.uint32))
        assert np.array_equal(idx["flags"] >> 4, stops[:valid].astype(np.uint8))
        one, one_info = D.index_stream(os_, s)
        assert one.tobytes() == idx.tobytes() and one_info.nBytes == info.nBytes
        if first_bad is None:
            assert info.nBytes == oracle.stream_info(os_, s)["nBytes"]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    print("\n%d streams, %d with a flagged frame, refused outright: %s" % (len(streams), flagged, dict(refused)))
    assert all(why in REFUSALS and REFUSALS[why] in text for why in refused)
    assert all(clause in text for clause in REFUSALS.values())
    assert flagged >= 180


@pytest.mark.parametrize("n_strided", [8, 9, 15, 16])
def test_a_frame_past_its_256_words(oracle, n_strided):
    """an OS93 Type 0 header with many strided bands: the index pass names no output index past the row's pad word (a batch made of
    its records used to be refused as inconsistent, and with sixteen strided bands the index wrapped in its nine bits), and
    the reference -- which has 512 words -- gives the restatement's PCM while its frames stay inside them"""
    c = C.past_the_row(n_strided)
    s = c.chans[0][1]
    idx, info = D.index_stream(c.os, s)
    assert info.nValidFrames == C.n_frames(s) == 6 and not idx["flags"].any()
    bands = 16 if n_strided == 16 else 15
    want = [min(1 + 32 * k if k <= n_strided else 1 + 32 * n_strided + 16 * (k - n_strided), 256) if k < bands else 0 for k in range(1, 16)]
    for r in idx:
        assert [int(x) & 0x1FF for x in r["split"]["state"]] == want
    assert C.overruns(c, 256) and C.overruns(c, 512) == (n_strided == 16) and not C.fatal(oracle, c)
    literal, _ = D.index_stream(c.os, s, literal=True)
    assert literal.tobytes() == idx.tobytes()
    if not C.checker_available():
        pytest.skip(C.MISSING)
    ref, = C.run_reference([c])
    if n_strided < 16:
        assert ref.kind == "decoded" and np.array_equal(ref.pcm, C.oracle_pcm(oracle, c))
