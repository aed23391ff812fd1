"""The even deal of 1994+ frames on the host (dcs_package.h): its rule, the mid records of the host index walk, and the
packages of both deals.  No GPU."""
import numpy as np
import pytest

import dcsexplorer_amd as D
import enc_ref
from util import make_stream, os_for

FORMATS_94 = [D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3]
SPLIT_MID, STRADDLE = 0x800, 0x200


@pytest.mark.parametrize("nbands", list(range(1, 17)))
def test_every_unit_once_and_in_order(nbands):
    """band 0, band 1 and two halves of every later band, dealt to eight lanes: consecutive ranges that cover all of them,
    ceil(units / 8) or one fewer each, the fuller lanes first"""
    units = nbands if nbands < 2 else 2 * nbands - 2
    at, counts = 0, []
    for q in range(8):
        first, count, _ = D.even_deal_lane(nbands, q)
        assert first == at and count >= 0
        at += count
        counts.append(count)
    assert at == units
    assert max(counts) == -(-units // 8) and min(counts) >= max(counts) - 1
    assert counts == sorted(counts, reverse=True)


# ---- an independent walk of a band, in Python, over the codebooks as csrc/dcs_tables.h lists them (read by tests/enc_ref.py
# for the encoder's reference): prefix codes matched bit by bit, nothing of the library's tables or readers in it
def _sample_books():
    books = {}
    for w in range(1, 7):
        books[w] = {(n, c): (2 if v & 0x80 else 1) for c, n, v in enc_ref._vlc("kVlc94Sample%d" % w)}
    return books


BOOKS = _sample_books()


def walk_to_middle(stream, fmt, rec, band):
    """-> (bits from the frame's first bit, output index, straddle) where the band stands at the first code boundary with at
    least half of its samples done; None for a band whose code the frame's record does not let a clean frame have"""
    hdr = stream[2:18]
    strided = (hdr[band] >> 6) & 1
    count, inc = (32 if band == 15 else 16) >> strided, 1 + strided
    half = count - count // 2
    bits = int(rec["split"]["bitDelta"][band - 1])
    idx = int(rec["split"]["state"][band - 1]) & 0x1FF
    code = int(rec["bandType"][band])
    if code == 0:
        return bits, idx + half, False                  # no code: the halved count is the band's advance
    if fmt != D.FMT_94_T0:
        code = int(enc_ref.XLAT[0 if band < 3 else 1 if band < 6 else 2][code]) & 0xFF
    if code > 6:
        return bits + half * code, idx + half * inc, False
    pos = (2 + 16) * 8 + int(rec["bitOff"]) + bits      # the stream's bit that starts the band
    done = 0
    while done < half:
        n = c = 0
        while (n, c) not in BOOKS[code]:
            c = (c << 1) | ((stream[pos >> 3] >> (7 - (pos & 7))) & 1)
            pos += 1
            n += 1
            assert n <= 16
        done += BOOKS[code][(n, c)]
    return pos - (2 + 16) * 8 - int(rec["bitOff"]), idx + done * inc, done > half


@pytest.mark.parametrize("fmt", FORMATS_94)
@pytest.mark.parametrize("nbands,stride_from,profile", [(16, 16, 0), (12, 16, 5), (12, 6, 1), (15, 3, 2), (13, 16, 3), (16, 12, 4)])
def test_mid_records_against_an_independent_walk(fmt, nbands, stride_from, profile):
    """every band of 16 or 32 samples of every frame: bits, output index and the straddle flag of the mid record equal what
    the walk above finds; the records proper are what dcs_index_stream makes"""
    s = make_stream(fmt, 24, seed=91000 + 100 * nbands + stride_from + fmt, profile=profile, stride_from=stride_from, nbands=nbands)
    idx, info, mids = D.index_stream_mids(os_for(fmt), s)
    idx2, _ = D.index_stream(os_for(fmt), s)
    assert idx.tobytes() == idx2.tobytes() and len(idx) == 24
    for f in range(len(idx)):
        assert idx["flags"][f] == 0 and mids[f, 0] == 1 and mids[f, 1] == 0
        for band in range(2, 16):
            m = int(mids[f, band])
            if band >= nbands:
                assert m == 0
                continue
            want = walk_to_middle(s, fmt, idx[f], band)
            assert (m & 0xFFFF, (m >> 16) & 0x1FF, bool((m >> 16) & STRADDLE)) == want, (f, band)
            assert (m >> 16) & ~0x3FF == 0


def test_the_streams_above_straddle_in_bands_other_than_15():
    """the set the walk is held against has two-zeros codes across the middle in bands 2 .. 14, coded and strided ones, in
    all three layouts -- found by the Python walk, not read off the records"""
    seen = {}
    for fmt in FORMATS_94:
        for nbands, stride_from, profile in [(12, 16, 5), (12, 6, 1), (13, 16, 3)]:
            s = make_stream(fmt, 24, seed=91000 + 100 * nbands + stride_from + fmt, profile=profile, stride_from=stride_from, nbands=nbands)
            idx, _ = D.index_stream(os_for(fmt), s)
            for f in range(len(idx)):
                for band in range(2, nbands):
                    if walk_to_middle(s, fmt, idx[f], band)[2]:
                        seen.setdefault(fmt, set()).add(band)
    assert all(len(seen.get(fmt, ())) >= 3 for fmt in FORMATS_94), seen
    strided = [b for fmt in seen for b in seen[fmt] if b >= 6]
    assert strided


def test_band_15_of_many_streams_equals_the_records_own():
    """the walk that makes the mid records reproduces, for band 15, what the index walk itself has always recorded --
    two-zeros codes across the middle included"""
    n = straddles = 0
    for k in range(24):
        fmt = FORMATS_94[k % 3]
        s = make_stream(fmt, 32, seed=92000 + k, profile=k % 6, stride_from=16 if k % 4 else 12)
        idx, info, mids = D.index_stream_mids(os_for(fmt), s)
        coded = (idx["bandType"][:, 15] != 0) & (idx["flags"] == 0) & (idx["nBands"] == 16)
        own = idx["split"]["prv"][:, 14].astype(np.uint32) | (idx["split"]["prvDelta"][:, 14].astype(np.uint32) << 16)
        assert np.array_equal(mids[coded, 15], own[coded])
        n += int(coded.sum())
        straddles += int(((own[coded] >> 16) & STRADDLE != 0).sum())
    assert n > 200 and straddles > 10


def test_flag_off_packages_are_todays():
    """without mid records the packer writes what it wrote before, byte for byte: dcs_pack_chunks is that path, and
    dcs_pack_chunks_mids with mids = None, or with the mids of frames that keep whole bands (sixteen bands), gives the same"""
    streams = [(os_for(fmt), make_stream(fmt, 20, seed=93000 + k, profile=k), 255, 0x64) for k, fmt in enumerate(FORMATS_94)]
    b = D.build_stream_batch(streams)
    for fpw in (4, 8, 16):
        plain = D.pack_chunks(b["blob"], np.asarray(b["srcs"]), b["jobs"], fpw)
        assert np.array_equal(D.pack_chunks(b["blob"], b["srcs"], b["jobs"], fpw, mids=b["srcs"].mids), plain)
    few = [(os_for(fmt), make_stream(fmt, 20, seed=93100 + k, profile=5, nbands=12), 255, 0x64) for k, fmt in enumerate(FORMATS_94)]
    b = D.build_stream_batch(few)
    for fpw in (4, 8, 16):
        plain = D.pack_chunks(b["blob"], np.asarray(b["srcs"]), b["jobs"], fpw)
        dealt = D.pack_chunks(b["blob"], b["srcs"], b["jobs"], fpw, mids=b["srcs"].mids)
        assert dealt.shape == plain.shape                       # (the split record keeps its size)
        assert np.array_equal(dealt, plain) == (fpw != 8)       # (the deal is for eight lanes per frame)
        if fpw == 8:
            # only the split records differ: bytes [8 x 80, 8 x 80 + 64 x 4)
            diff = np.nonzero((dealt != plain).any(axis=0))[0]
            assert diff.min() >= 640 and diff.max() < 640 + 256


def test_split_records_of_the_even_deal():
    """lane q's record names the band of its first unit, the mid flag exactly when that unit is a second half, and the bits
    and output index of the band's or the mid record"""
    for nbands in (5, 9, 12, 13, 15):
        s = make_stream(D.FMT_94_T1_S3, 8, seed=94000 + nbands, profile=5, nbands=nbands)
        b = D.build_stream_batch([(D.OS94, s, 255, 0x64)])
        pk = D.pack_chunks(b["blob"], b["srcs"], b["jobs"], 8, mids=b["srcs"].mids)
        split = pk[0, 640:640 + 256].view(np.uint32).reshape(8, 8)             # [q][slot]
        for slot in range(8):
            rec, mids = b["srcs"]["idx"][slot], b["srcs"].mids[slot]
            for q in range(1, 8):
                first, count, _ = D.even_deal_lane(nbands, q)
                w = int(split[q, slot])
                if count == 0:
                    assert w & 0x8000
                    continue
                band, half = (first, 0) if first < 2 else (1 + first // 2, first & 1)
                assert (w >> 28) == band and bool((w >> 16) & SPLIT_MID) == bool(half)
                if half:
                    assert (w & 0x7FFF) == (int(mids[band]) & 0xFFFF) and ((w >> 16) & 0x3FF) == ((int(mids[band]) >> 16) & 0x3FF)
                else:
                    assert (w & 0x7FFF) == int(rec["split"]["bitDelta"][band - 1])
                    assert ((w >> 16) & 0x1FF) == int(rec["split"]["state"][band - 1]) & 0x1FF
