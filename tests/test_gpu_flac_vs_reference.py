"""dcs_flac_decode and dcs_encode_files on the MI355X against the compiled libnyquist / libFLAC (oracle/_ref/dcs_flacref,
`make -C oracle flacref`) and the restatement, on the seeded files of tests/flac_fuzz_cases.py.  F1 loads dwords aligned to
the uploaded bytes, so a frame's alignment is set by everything before it in the call: every set runs as generated, shuffled
with fillers of other lengths between its files, and a few files alone.  The damaged files (each behind a good one) are held
to the relation below; every one of them has passed the library's own walk on the host under AddressSanitizer and UBSan
(tools/flac_walk_sanitize.sh) before it came here."""
import collections
import re

import numpy as np
import pytest

import dcsexplorer_amd as D
import flac_fuzz_cases as Z
import flac_ref as R
import wav_cases as W
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_INVALID_ARG, DcsError

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not Z.checker_available(), reason=Z.MISSING)]


def same_bits(a, b):
    return len(a) == len(b) and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def kept(load):
    return load.kind == "loaded" and not load.reports


@pytest.fixture(scope="module")
def well():
    """[(case, the checker's verdict, flac_ref's mono floats)]; computed once, never changed"""
    cases = Z.well_formed()
    return list(zip(cases, Z.check_load([c.data for c in cases]), [R.decode(c.data)[1] for c in cases]))


def test_well_formed_in_three_compositions(gpu_ctx, well):
    """bit for bit against flac_ref on every file and against the checker's floats (downmixed as EncodeFile does) on every
    kept one, in each composition"""
    fill = Z.fillers()
    fill_want = [R.decode(b)[1] for b in fill]
    n_checker = 0
    for what, order, lead in Z.compositions(len(well), 0):
        files, expect = [], []
        for i, k in zip(order, lead):
            for j in range(k):
                files.append(fill[(i + j) % 3])
                expect.append((None, None, fill_want[(i + j) % 3]))
            files.append(well[i][0].data)
            expect.append(well[i])
        got = gpu_ctx.flac_decode(files)
        assert len(got) == len(files)
        for y, (c, l, want) in zip(got, expect):
            name = c.name if c else "filler"
            assert same_bits(y, want), (what, name)
            if c is not None and kept(l) and l.values is not None:
                assert same_bits(y, R.downmix(l.values, c.fmt[1])), (what, name)
                n_checker += 1
    assert n_checker >= 2 * 0.9 * len(well) - 2


@pytest.mark.parametrize("bits", [16, 24])
def test_flac_equals_wav_of_the_same_integers(gpu_ctx, well, bits):
    """encode_files(at_unity=True) on the kept files of one depth and on the WAV files of the same integers: the same bytes.
    The set is the quiet files (|x| <= 0.4): the converter overshoots a full-scale signal past 1, which the encoder refuses
    for FLAC and WAV alike (rule 12), and the limit-driven files are full scale on purpose; and both forms of
    each pass the host's plan"""
    quiet = [c for c, l, want in well if kept(l) and c.fmt[2] == bits and np.abs(want).max() <= 0.4]
    wav_of = lambda c: W.wav("s16" if bits == 16 else "s24", c.fmt[1], c.fmt[0], R.cut(c.ints, bits))
    # (the host plan refuses a file under 64 bytes and one that resamples to no samples, whatever its format)
    plan = [D.encode_files_plan([c.data, wav_of(c)], at_unity=True)[2] for c in quiet]
    keep = [c for c, st in zip(quiet, plan) if not np.any(st)][:40]
    assert len(keep) >= 25
    flacs, wavs = [c.data for c in keep], [wav_of(c) for c in keep]
    a, ai = gpu_ctx.encode_files(flacs, at_unity=True)
    w, wi = gpu_ctx.encode_files(wavs, at_unity=True)
    assert a == w
    assert list(ai["nSamples"]) == list(wi["nSamples"]) and set(wi["kind"]) == {D.FILE_WAV} and set(ai["kind"]) == {D.FILE_FLAC}


def test_damaged_files(gpu_ctx, well):
    """one call per damaged file, its well-formed source in front.
      the checker threw                          -> the library refuses (BAD_STREAM or INVALID_ARG), dcs_last_error names file 1,
                                                    and the context then decodes the good file correctly
      the checker loaded, clean, library accepts -> equal bits
      the checker loaded, library refuses        -> flac_ref refuses too, same status and frame, under a named clause of
                                                    INTEGRATION.md "Encoding files" rules 20-25 that is stricter than libFLAC
      the checker crashed or the screen reported -> no claim rests on the reference
      always                                     -> the library does what flac_ref predicts: status, frame, or bits"""
    damaged = Z.damaged()
    loads = Z.check_load([d.data for d in damaged])
    tally, codes, clauses = collections.Counter(), collections.Counter(), collections.Counter()
    for d, l in zip(damaged, loads):
        src, _, good_want = well[d.source]
        p = Z.predict(d.data)
        try:
            got = gpu_ctx.flac_decode([src.data, d.data])
            status, msg = 0, ""
        except DcsError as e:
            status, msg = e.status, gpu_ctx.L.dcs_last_error(gpu_ctx.h).decode()
        assert status == p["status"], (d.name, status, msg, p)
        if status == 0:
            assert same_bits(got[0], good_want), d.name
            assert same_bits(got[1], R.decode(d.data)[1]), d.name
        else:
            assert status in (ERR_BAD_STREAM, ERR_INVALID_ARG) and msg.startswith("file 1:"), (d.name, msg)
            m = re.search(r"frame (\d+)", msg)
            if p["frame"] is not None:
                assert m and int(m.group(1)) == p["frame"], (d.name, msg, p)
            assert same_bits(gpu_ctx.flac_decode([src.data])[0], good_want), d.name
            if p["where"] == "device":
                codes[p["code"]] += 1
            else:
                tally["refused by the host index"] += 1
        if l.kind == "threw":
            assert status != 0, (d.name, l.text)
            tally["checker threw, refused"] += 1
        elif kept(l) and status == 0:
            assert same_bits(got[1], R.downmix(l.values, src.fmt[1])), d.name
            tally["accepted and equal"] += 1
        elif kept(l):
            clause = Z.stricter_clause(p)
            assert clause is not None, (d.name, msg, p)
            clauses[clause] += 1
        else:
            tally["checker crashed or screen reported"] += 1
    print("\ndamaged: %d files" % len(damaged), dict(tally), "\ndevice codes:", dict(codes), "\nstricter than libFLAC:", dict(clauses))
    assert all(codes[c] >= 5 for c in Z.CODES), codes
    assert tally["refused by the host index"] >= 20 and tally["accepted and equal"] >= 20, tally
