"""The encoder restatements (tests/enc_ref.py, tests/enc93_ref.py) against the compiled reference encoder
(oracle/_ref/dcs_encref, `make -C oracle encref`) on seeded adversarial cases (tests/enc_cases.py): denormal and
underflowing signals, -0.0, full scale, frame-edge impulses, Nyquist squares, and every edge of CompressionParams, in every
layout of both encoder families.  The restatements are what the GPU encoders are fuzzed against at scale, so they must not
share a misreading with the kernels: here they answer to the reference itself."""
import pytest

import enc_cases as C

SEED = 0xE4CF
N_SETS = 200                # x 10 cases, + one 65 535-frame stream per family


@pytest.fixture(scope="module")
def results():
    if not C.reference_available():
        pytest.skip(C.MISSING)
    res = C.check_all(C.keys(SEED, N_SETS))
    print("\nrestatement vs reference, per layout:\n" + C.format_tally(C.tally(res)))
    return res


def test_restatement_equals_reference_bytes(results):
    bad = []
    for r in results.values():
        if r.status == "dropped" or r.want == r.ref:
            continue
        # the only licensed difference: the library's Keep +15 rule (OS93 Type 1), which must then have fired
        if not (r.family != "94" and r.fired > 0):
            first = next((i for i, (a, b) in enumerate(zip(r.want, r.ref)) if a != b), min(len(r.want), len(r.ref)))
            bad.append("%s: %d vs %d bytes, first difference at byte %d" % (r.name, len(r.want), len(r.ref), first))
    assert not bad, "%d cases differ from the reference:\n%s" % (len(bad), "\n".join(bad[:20]))


def test_winner_and_bands_to_keep_match_the_reference_header(results):
    for r in results.values():
        if r.status != "kept":
            continue
        keep, facts = C.header_facts(r.family, r.ref)
        assert r.keep == keep, r.name
        assert r.ref[:2] == r.want[:2], r.name
        typ, sub = r.win
        want = {"type": typ, "sub&2": sub & 2, "sub&1": sub & 1}
        assert all(want[k] == v for k, v in facts.items()), (r.name, r.win, facts)


def test_the_screen_is_not_hollow(results):
    t = C.tally(results)
    kept = sum(c["kept"] for c in t.values())
    assert kept >= 0.9 * len(results), C.format_tally(t)
    for fl, c in t.items():
        assert c["kept"] >= 20, (fl, C.format_tally(t))
    assert all(r.status == "kept" for r in results.values() if r.name.startswith("longest/")), "a 65 535-frame stream was not kept"
