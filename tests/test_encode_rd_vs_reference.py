"""The rate-distortion 1994+ encoder against the references, without a GPU: every stream the numpy restatement
(tests/enc94rd_ref.py) writes goes through the compiled reference decoder and the oracle to its last bit, and their frame
buffers are the reconstruction the search assumed; the cases reach what they were made for; the reference ENCODER's own
choice is a point of the searched space and never beats the trellis on its own header; and the quality condition: within
the reference-equal stream's bytes, no more time-domain error than that stream has."""
import numpy as np
import pytest

import enc94rd_cases as C
import enc94rd_ref as R
import sweep_ref as S

E = R.E
OS94, OS95 = 2, 3


@pytest.mark.parametrize("name,fmt,rate,mqe", C.GRID, ids=C.IDS)
def test_decoders_read_the_stream_to_its_last_bit(reference, oracle, dcs, name, fmt, rate, mqe):
    s, ch, rec, codes = C.expected(name, fmt, rate, mqe)
    t = C.analysis(name)["t"]
    F = C.FRAMES[name]
    assert len(s) == 18 + (ch["frameBits"] + 7) // 8 and (s[0] << 8 | s[1]) == F
    # the sub-type bits ride in header bytes 1 and 2, and a band the header cuts has them set: a Type 0 stream of fewer than
    # three bands reads 1 or 3 there whatever was asked for (no decoder looks: Type 0 has no sub-types, and the reference's
    # encoder writes the same); Type 1 sub-type 0 keeps at least three bands, so that its bits are the ones written
    cut = (2 if ch["numBands"] < 2 else 0) | (1 if ch["numBands"] < 3 else 0)
    assert (s[2] >> 7, (s[3] >> 7) << 1 | s[4] >> 7) == (ch["type"], ch["sub"] | cut)
    assert ch["type"] == 0 or ch["sub"] == 3 or cut == 0
    assert all((s[2 + b] & 0x7F) != 0x7F for b in range(ch["numBands"])) and all(v == 0xFF for v in s[2 + ch["numBands"]:18])
    os_ = OS95 if ch["sub"] == 3 else OS94
    probe = C.closing_probe(s, ch, codes)
    for checker in (reference, oracle):
        out, offs, types, stops = checker.decompress(os_, probe, R.M0, F + 1)
        assert not stops.any()
        assert offs[F] - offs[0] == ch["frameBits"]
        fb = out[:F, :256].astype(np.int16).astype(np.int64)
        assert np.array_equal(fb, R.frame_buffer(rec))
        assert not out[:F, 256:].any()
        assert int(((R.frame_buffer(t) - fb) ** 2).sum()) == ch["sqErr"]
        assert np.array_equal(types[:F].astype(np.int64), codes)
    idx, si = dcs.index_stream(os_, s)
    assert si.nFrames == F and len(idx) == F
    assert np.array_equal(idx["bitOff"].astype(np.int64) - int(idx["bitOff"][0]), offs[:F] - offs[0])


def test_cases_reach_what_they_are_for():
    """Reached by the grid: in Type 1 every band-type code 0..15 in each of the three band classes (bands 0-2, 3-5, 6-15);
    every pre-adjust value of both sub-types; an odd and an even zero run under each Huffman width; raw widths, the 8 bits of
    code 15 in bands 0-2 among them; numBands 1 and 16; two streams nothing fits; a first frame that wants code 15 and is
    refused the step."""
    seen = {0: set(), 1: set(), 2: set()}
    pre = {0: set(), 3: set()}
    runs = {w: set() for w in range(1, 7)}
    raw, bands, misfits, wanted15 = set(), set(), 0, 0
    for g in C.GRID:
        s, ch, rec, codes = C.expected(*g)
        an = C.analysis(g[0])
        typ, sub, n = ch["type"], ch["sub"], ch["numBands"]
        bands.add(n)
        misfits += not ch["fits"]
        prev = np.vstack([np.zeros((1, 16), np.int64), codes[:-1]])
        for b in range(n):
            pm = R.pre_map(typ, sub, b)[prev[:, b]]
            if typ == 1:
                seen[0 if b < 3 else 1 if b < 6 else 2] |= set(codes[:, b].tolist())
                if b < 3:
                    pre[sub] |= set(pm[codes[:, b] > 0].tolist())
                # the first frame of a chain of this band: is code 15's item (were the step 0 -> 15 allowed) better than every
                # allowed code's?  Then the chain at lambda = 0 wants the step, and the trellis refuses it
                tr, hwin, _ = R.search(an, g[3], (typ, sub))
                for k in range(R.NH):
                    w, sc, ok = R.options(1, b, int(hwin[b, k]), 0)
                    d = np.maximum(an["D"][0, b, w, sc], R.band_floor(g[3])[b])
                    if ok[15] and d[15] < d[:15][ok[:15]].min():
                        wanted15 += 1
                        assert R.path(tr, b, k, 0)[0] != 15 and R.HDR_BITS[0, 15] < 0
            w, sc, _ = E.interpret(typ, b, codes[:, b], s[2 + b] & 0x3F, pm)
            for f in range(codes.shape[0]):
                if w[f] > 6:
                    raw.add(int(w[f]))
                elif w[f] >= 1:
                    q = np.clip(an["Q0"][f, R.FIRST[b]:R.FIRST[b] + R.COUNT[b], sc[f]], -(1 << (w[f] - 1)), (1 << (w[f] - 1)) - 1)
                    run = 0
                    for v in list(q) + [1]:
                        if v == 0:
                            run += 1
                        elif run:
                            runs[int(w[f])].add(run & 1)
                            run = 0
    assert seen[0] == seen[1] == seen[2] == set(range(16))
    assert pre == {0: {0, 1}, 3: {0, 1, 2, 3, 4}}
    assert all(r == {0, 1} for r in runs.values())
    assert {7, 8} <= raw and {1, 16} <= bands and misfits >= 2 and wanted15 >= 1


@pytest.mark.parametrize("name", ["music", "noise_m40", "level_step"])
def test_the_reference_encoder_is_a_point_of_the_space(name):
    """the reference's own (header, codes), priced with the restatement's items where it quantises without wrapping, costs
    no less than the trellis's optimum for that header, at every ladder entry"""
    an = C.analysis(name)
    D, B = an["D"], an["B"]
    f, lo, hi, (ps, rlo, rhi) = E.analyse_stream(an["x"])
    Eb = R.band_floor(C.MQE)
    lam = np.array(R.LADDER, dtype=object)
    priced = 0
    for typ, sub in R.LAYOUTS:
        hdr, keep, _ = E.header(ps, rlo, rhi, typ, sub)
        codes = E.choose_codes(f, lo, hi, hdr, keep, typ, sub)
        hwin = np.repeat((hdr.astype(np.int64) & 0x3F)[:, None], R.NH, axis=1)
        tr = R.trellis(D, B, typ, sub, hwin, Eb)
        prev = np.vstack([np.zeros((1, 16), np.int64), codes[:-1]])
        for b in range(keep):
            pre = R.pre_map(typ, sub, b)[prev[:, b]]
            w, sc, _ = E.interpret(typ, b, codes[:, b], int(hwin[b, 0]), pre)
            smp = f[:, R.FIRST[b]:R.FIRST[b] + R.COUNT[b]]
            scaled = E.round_away(smp * np.float32(32768) / E.SCALE[np.minimum(sc, 63)].astype(np.float32)[:, None])
            half = (1 << np.maximum(w - 1, 0))[:, None]
            if ((w[:, None] > 0) & ((scaled < -half) | (scaled > half - 1))).any():
                continue                                        # the reference wrapped a sample in this band
            fr = np.arange(len(w))
            d, bits = D[fr, b, w, sc], B[fr, b, w, sc] + R.HDR_BITS[prev[:, b], codes[:, b]]
            assert (R.HDR_BITS[prev[:, b], codes[:, b]] >= 0).all() and (sc <= 0x3F).all()
            cost = int(np.maximum(d, Eb[b]).sum()) + lam * int(bits.sum())
            assert all(int(tr["J"][b, 0, li]) <= cost[li] for li in range(R.KL)), (typ, sub, b)
            priced += 1
    assert priced >= 8


QUALITY = sorted(C.quality_signals())


@pytest.mark.parametrize("name", QUALITY)
def test_quality_within_the_reference_streams_bytes(oracle, name, capsys):
    """B and E of the reference-equal stream (enc_ref; sweep_ref.measure on the oracle's decode); this encoder with
    budgetBytes = B writes at most B bytes with an error of at most E: every layout, every rate of sweep_ref.RATES"""
    an = C.quality_analysis(name)
    x = E.to_float(C.quality_signals()[name])
    rows, bad = [], []
    for lay in C.QUALITY_LAYOUTS:
        for rate in S.RATES:
            Bref, Eref = C.quality_reference(oracle, name, lay, rate)
            s, ch, _, _ = R.encode(an, lay, Bref)
            err = C.time_error(oracle, OS95 if lay[1] == 3 else OS94, x, s)
            rows.append("%-18s (%d,%d) %6d: B %5d E %12d | %5d %12d" % (name, lay[0], lay[1], rate, Bref, Eref, len(s), err))
            if not (len(s) <= Bref and err <= Eref):
                bad.append(rows[-1])
    with capsys.disabled():
        print("\n" + "\n".join(rows))
    assert not bad, bad
