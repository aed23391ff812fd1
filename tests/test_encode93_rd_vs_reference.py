"""The rate-distortion OS93 Type-0 encoder against the reference encoder, without a GPU: the quality condition.  For every
recording whose PCM tests/golden/encoder_golden.npz carries and the seeded ec_* signals, each cut to 64 frames, at the six
rates of sweep_ref.RATES and for both versions: B and E are the bytes and the time-domain error (sweep_ref.measure on the
oracle's decode) of the reference-equal Type-0 stream (tests/enc93_ref.py, and the compiled reference encoder's where it is
built); this encoder with budgetBytes = B fits, and its error is never higher.

POLARITY.  The OS93 decoders' transform returns a frame buffer's PCM with its polarity turned: the decode of a recording's
reference-equal stream correlates with its source at -0.99 (256 kbit/s) to -0.93 (48 kbit/s); DESIGN.md 10.10 found the
same, -0.991.  This encoder's targets are therefore the NEGATED spectrum, and its decode has the source's
polarity.  sweep_ref.measure compares sample with sample, so the reference-equal stream's E is about 4 sum x^2 whatever its
coding noise, and the condition as the issue states it (test_quality_within_the_reference_streams_bytes) holds in all 108
cases by a wide margin, median ratio 0.0075: it says little about the search.  The comparison that does is
test_quality_against_the_reference_stream_with_its_polarity_taken_out: this encoder's E against the reference-equal stream's
with ITS decode negated before it is measured, noise against noise.  There the error is never higher in 104 of 108 cases,
median ratio 0.55, and the four that miss are named with their two errors."""
import tempfile

import numpy as np
import pytest

import enc93_ref as O
import enc93rd_cases as C
import enc93rd_ref as R
import enc_cases as X
import sweep_ref as S

QUALITY = sorted(C.quality_signals())
_ROWS = {}


def _errors(oracle, version, x, stream):
    """(E, E with the decode negated before it is measured)"""
    nf = (stream[0] << 8) | stream[1]
    d = np.asarray(oracle.decode(R.OS_OF[version], 255, [stream], [255], nf + 1)).astype(np.int64)
    return S.sq_err(S.measure(x, d)), S.sq_err(S.measure(x, -d))


def rows(oracle, name):
    """per (version, rate): dict(B, E, En of the reference-equal stream(s); bytes, err, errn, fits of this encoder's),
    computed once per process"""
    if name in _ROWS:
        return _ROWS[name]
    x = R.E.to_float(C.quality_signals()[name])
    out = []
    for version in (C.A, C.B):
        an = C.quality_analysis(name, version)
        for rate in S.RATES:
            refs = [O.encode(x, version, 0, targetBitRate=rate)[0]]
            if X.reference_available():
                case = X.Case(name, x, "93", "T0", version, 0, -1, dict(R.DEFAULTS, targetBitRate=rate))
                with tempfile.TemporaryDirectory() as tmp:
                    refs.append(X.run_reference(X.EXE, case, tmp)[0])
            for ref in dict.fromkeys(refs):
                Eref, Enref = _errors(oracle, version, x, ref)
                s, ch, _, _ = R.encode(an, len(ref))
                err, errn = _errors(oracle, version, x, s)
                out.append(dict(version=version, rate=rate, B=len(ref), E=Eref, En=Enref, bytes=len(s), err=err, errn=errn, fits=ch["fits"]))
    _ROWS[name] = out
    return out


def _table(name, rs, a, b):
    return ["%-18s %x %6d: B %5d E %13d -> %5d %13d" % (name, r["version"], r["rate"], r["B"], r[a], r["bytes"], r[b]) for r in rs]


@pytest.mark.parametrize("name", QUALITY)
def test_quality_within_the_reference_streams_bytes(oracle, name, capsys):
    """the condition as the issue states it: fits, and sweep_ref.measure's error on the oracle's decode is never higher than
    the reference-equal stream's (whose decode has its polarity turned: this file's docstring)"""
    rs = rows(oracle, name)
    with capsys.disabled():
        print("\n" + "\n".join(_table(name, rs, "E", "err")))
    bad = [r for r in rs if not (r["fits"] and r["bytes"] <= r["B"] and r["err"] <= r["E"])]
    assert not bad, _table(name, bad, "E", "err")


# the cases that miss against the reference-equal stream with its polarity taken out: (signal, version, rate) -> (that
# stream's error, this encoder's).  All four are the quietest signal at the two highest rates: maximumQuantizationError at
# its default is the floor below which this encoder spends no bits (3 676 bytes of the 7 485 and 6 868 allowed), and the
# reference spends them
KNOWN = {("ec_music0", C.A, 256000): (280829882, 331907262), ("ec_music0", C.A, 192000): (293823827, 331907262),
         ("ec_music0", C.B, 256000): (281026454, 331808848), ("ec_music0", C.B, 192000): (294038586, 331808848)}


@pytest.mark.parametrize("name", QUALITY)
def test_quality_against_the_reference_stream_with_its_polarity_taken_out(oracle, name, capsys):
    """the same B, the same streams; the reference-equal stream's decode negated before sweep_ref.measure, this encoder's
    measured as it comes: the error is never higher, but for the cases of KNOWN, which are held to their figures"""
    rs = rows(oracle, name)
    with capsys.disabled():
        print("\n" + "\n".join(_table(name, rs, "En", "err")))
    bad = []
    for r in rs:
        key = (name, r["version"], r["rate"])
        assert r["fits"] and r["bytes"] <= r["B"]
        assert r["err"] <= r["errn"]                                # this encoder's decode has the source's polarity (a silent one: equal)
        if key in KNOWN:
            assert (r["En"], r["err"]) == KNOWN[key] or r["err"] <= r["En"], key
        elif r["err"] > r["En"]:
            bad.append(r)
    assert not bad, _table(name, bad, "En", "err")


def test_known_misses_are_few():
    assert len(KNOWN) * 20 <= len(QUALITY) * 2 * len(S.RATES)       # at most 5 % of the grid
    assert len(QUALITY) * 2 * len(S.RATES) == 108
