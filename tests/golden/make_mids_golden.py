#!/usr/bin/env python3
"""Generates mids_golden.json: per case of tests/mids_cases.py the SHA-256 of (records, StreamInfo bytes, mid records) as
index_stream_mids returns them.  Made with the library of the commit BEFORE the index walk recorded the middles itself (the
mid records then came from a second walk over every frame's record), so the fixture pins that commit's outputs.  The
generator asserts that the cases exercise what they are there for: two-zeros codes across the middle of bands other than 15,
frames that end in error behind valid ones, every sample codebook and a raw width in a first half."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dcsexplorer_amd as D             # noqa: E402
import enc_ref                          # noqa: E402
import mids_cases as C                  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    golden = {}
    straddles = stopped = 0
    widths = set()
    for name, os_, s in C.cases():
        idx, info, mids = D.index_stream_mids(os_, s)
        golden[name] = C.digest(idx, info, mids)
        if info.format < D.FMT_94_T0:
            assert not mids.any(), name
            continue
        straddles += int((((mids[:, 2:15] >> 16) & C.STRADDLE) != 0).sum())
        stopped += int(len(idx) >= 2 and idx["flags"][-1] != 0)
        for f in np.nonzero(idx["flags"] == 0)[0]:
            assert mids[f, 0] == 1, (name, f)
            for band in range(2, int(idx["nBands"][f])):
                code = int(idx["bandType"][f, band])
                if code and info.format != D.FMT_94_T0:
                    code = int(enc_ref.XLAT[0 if band < 3 else 1 if band < 6 else 2][code]) & 0xFF
                widths.add(code)
        assert not mids[idx["flags"] != 0].any(), name
    print("%d cases, %d straddles outside band 15, %d streams stopped in error behind a valid frame, widths %s"
          % (len(golden), straddles, stopped, sorted(widths)))
    assert straddles >= 20 and stopped >= 20
    assert set(range(1, 7)) <= widths and any(w >= 7 for w in widths)
    json.dump(dict(cases=golden), open(os.path.join(HERE, "mids_golden.json"), "w"), indent=0)


if __name__ == "__main__":
    sys.exit(main())
