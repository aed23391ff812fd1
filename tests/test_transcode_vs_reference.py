"""The transcoding restatement (tests/transcode_ref.py) against the compiled reference composition on seeded cases
(tests/transcode_cases.py): every source layout into every target, at the recipe's volume and level and off it (clipping,
all-zero PCM, a low level), with the reference's CompressionParams and with their edges.  The oracle's recipe PCM must be the
compiled reference decoder's, and the restatement's bytes the reference encoder's on every case the enc_cases screen keeps.
The GPU module (test_gpu_transcode_vs_reference.py) holds the library to the same expectations."""
import pytest

import transcode_cases as X

SEED = 0x7C0D
N_SETS = 540                # 3 000-odd sources, ~2 700 of them re-encoded
N_DROPPED = 9               # the OS93a all-bands-dropped stream, once per target


@pytest.fixture(scope="module")
def results():
    if not X.reference_available():
        pytest.skip("oracle/_ref not built (needs the reference sources; `make -C oracle ref encref`)")
    res = X.expect_all(X.keys(SEED, N_SETS, N_DROPPED))
    print("\ntranscoding restatement vs reference, re-encoded sources by source layout x target:\n" + X.format_tally(X.tally(res)))
    return res


def test_recipe_pcm_is_the_reference_decoders(results):
    bad = [e.name for es in results.values() for e in es if e.status not in ("copied", "bad") and not e.pcm_same]
    assert not bad, "%d sources decode differently:\n%s" % (len(bad), "\n".join(bad[:20]))


def test_restatement_equals_the_reference_composition(results):
    bad = []
    for es in results.values():
        for e in es:
            if e.status == "kept" and e.want != e.ref:
                first = next((i for i, (a, b) in enumerate(zip(e.want, e.ref)) if a != b), min(len(e.want), len(e.ref)))
                bad.append("%s: %d vs %d bytes, first difference at byte %d" % (e.name, len(e.want), len(e.ref), first))
            # the only licensed difference: the Keep +15 rule, OS93 targets only
            assert e.status != "rule" or (e.target[0] != 0x9400 and e.fired > 0), e.name
    assert not bad, "%d sources differ from the reference:\n%s" % (len(bad), "\n".join(bad[:20]))


def test_copies_and_bad_sources_follow_the_rule(results):
    n_bad = 0
    for key, es in results.items():
        for e in es:
            if e.status == "bad":
                n_bad += 1
        if key[0] == "dropped":
            st = [e.status for e in es if e.name.split("/")[1].startswith("enc-93a")]
            # copied for an OS93a target, re-encoded (and refused) for any other
            assert st == (["copied"] if es[0].target[0] == 0x9301 else ["bad"]), (key, st)
    assert n_bad >= 8


def test_the_screen_is_not_hollow(results):
    t = X.tally(results)
    checked = sum(c["kept"] + c["rule"] + c["dropped"] for c in t.values())
    kept = sum(c["kept"] for c in t.values())
    assert checked >= 1000 and kept >= 0.9 * checked, X.format_tally(t)
    for cell, c in t.items():
        assert c["kept"] >= 10, (cell, X.format_tally(t))
    # every path's sources are among them: flagged ones, encoder-made ones, recordings, every volume and level
    names = [e.name for es in results.values() for e in es if e.status == "kept"]
    for part in ("/synth-", "/large-", "/truncated-", "/enc-", "/rec-", "+tail"):
        assert sum(part in n for n in names) >= 10, part
    sets = [X.set_of(k) for k in results]
    for vl in ((0x67, 0xFF), (0xFF, 0xFF), (0, 0xFF), (1, 0xFF)):
        assert sum((s.volume, s.level) == vl for s in sets) >= 10, vl
    assert sum(s.volume == 0x67 and s.level < 0x67 for s in sets) >= 10
    assert sum(s.dcsa for s in sets) >= 10 and sum(s.params != sets[0].params for s in sets) >= 100
