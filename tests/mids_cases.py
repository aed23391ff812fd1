"""The streams that hold the mid records of the host index walk in place (tests/golden/make_mids_golden.py makes the fixture
from them, tests/test_index_mids_one_walk.py holds the built library against it): seeded synthetic streams, whole and damaged."""
import hashlib
import random

import dcsexplorer_amd as D
from util import os_for

FORMATS_94 = [D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3]
FORMATS_93 = [D.FMT_93_T0, D.FMT_93A_T1, D.FMT_93B_T1]
NBANDS = (2, 3, 8, 12, 15, 16)
STRIDE_FROM = (2, 9, 16)
PROFILES = (5, 3)           # the survey's code statistics; every code of the layout, raw widths among them
ZERO_PROFILE = 2            # four bands in ten without a code
STRADDLE = 0x200


def _whole():
    for fmt in FORMATS_94:
        for nbands in NBANDS:
            for stride_from in STRIDE_FROM:
                for profile in PROFILES:
                    seed = 0x31D5000 + 10000 * fmt + 100 * nbands + 10 * stride_from + profile
                    yield ("f%d_b%d_s%d_p%d" % (fmt, nbands, stride_from, profile), fmt,
                           D.synth_stream(fmt, 6, seed, nbands=nbands, stride_from=stride_from, profile=profile))
                    if stride_from == 2:        # (band 15 strided at 16 bands) ... and with bands whose bandType is 0
                        yield ("f%d_b%d_s2_p%d_zero" % (fmt, nbands, profile), fmt,
                               D.synth_stream(fmt, 6, seed + 500000, nbands=nbands, stride_from=2, profile=ZERO_PROFILE))
    for fmt in FORMATS_93:
        nbands = 18 if fmt == D.FMT_93A_T1 else 16
        yield ("f%d_1993" % fmt, fmt, D.synth_stream(fmt, 6, 0x31D5900 + fmt, nbands=nbands, profile=0))


def _damaged():
    rng = random.Random(0x31D5)
    shorts = [(fmt, D.synth_stream(fmt, 3, 0x31D5A00 + fmt, nbands=nbands, stride_from=stride_from, profile=profile))
              for fmt, nbands, stride_from, profile in zip(FORMATS_94, (8, 6, 5), (16, 3, 4), (5, 3, 0))]
    for fmt, s in shorts:
        for n in range(3, len(s) + 1):
            yield ("f%d_cut%d" % (fmt, n), fmt, s[:n])
    for k in range(200):
        fmt, s = shorts[k % 3]
        at = rng.randrange(2, len(s))
        b = bytearray(s)
        b[at] ^= rng.randrange(1, 256)
        yield ("f%d_flip%d_at%d" % (fmt, k, at), fmt, bytes(b))


_CASES = None


def cases():
    """-> [(name, os, stream bytes)], made once"""
    global _CASES
    if _CASES is None:
        _CASES = [(name, os_for(fmt), s) for name, fmt, s in list(_whole()) + list(_damaged())]
        assert len({c[0] for c in _CASES}) == len(_CASES)
    return _CASES


def digest(records, info, mids):
    return hashlib.sha256(records.tobytes() + bytes(info) + mids.tobytes()).hexdigest()
