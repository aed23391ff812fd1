#!/usr/bin/env python3
"""Generates the fixture of the FLAC writer on streams of any length (build container only; the output is data):
  flac_write_any_golden.json  per case of tests/flac_write_any_cases.py, with and without the MD5, at 48 000 Hz: the sha256
                              and the size of the file tests/flac_write_any_ref.py writes and its counts of block kinds;
                              the same for a subset of the cases at 4 000, 44 100 and 65 535 Hz; for the ragged list the
                              sha256 of the streams' concatenation, its size and the summed counts
Every file is first decoded by the vendored libFLAC, as make_flac_write_golden.py does it: libnyquist is built in a temp
dir, flac_write/fw_driver.c is linked against the archive's libFLAC and runs FLAC__stream_decoder over each file with MD5
checking on.  The generator asserts that libFLAC accepts every file, that the decoded samples equal the source and that
the MD5 check passes (for the files written without an MD5, libFLAC has nothing to compare and the first two hold).  There
are no exclusions: a failing case means the rule or the restatement is wrong.
"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import flac_write_any_cases as C                # noqa: E402
import flac_write_any_ref as A                  # noqa: E402
import make_encode_file_golden as MG            # noqa: E402
from oracle import flacref                      # noqa: E402  (libnyquist's build: one recipe)

HERE = MG.HERE
KINDS = ("nBlocks", "nConstant", "nVerbatim", "nFixed")


def entries():
    """-> [([(flac bytes, pcm)], record)]"""
    out = []
    for md5 in (True, False):
        for rate, cases in [(C.RATE, C.cases())] + [(r, C.subset()) for r in C.RATES]:
            for name, pcm in cases:
                b, info = A.write(pcm, rate, md5)
                rec = dict(name=name, rate=rate, md5=md5, sha256=hashlib.sha256(b).hexdigest(), bytes=len(b), **{k: info[k] for k in KINDS})
                out.append(([(b, pcm)], rec))
        written = [A.write(p, C.RATE, md5) for p in C.ragged()]
        kinds = {k: sum(w[1][k] for w in written) for k in KINDS}
        blob = b"".join(w[0] for w in written)
        rec = dict(name="ragged300", rate=C.RATE, md5=md5, streams=len(written), sha256=hashlib.sha256(blob).hexdigest(), bytes=len(blob), **kinds)
        out.append(([(w[0], p) for w, p in zip(written, C.ragged())], rec))
    return out


def main():
    C.check_tally()
    es = entries()
    with tempfile.TemporaryDirectory() as tmp:
        nq_lib = flacref.build_libnyquist(MG.NQ, os.path.join(tmp, "nq"))
        exe = os.path.join(tmp, "fw_driver")
        subprocess.check_call(["g++", "-O2", "-w", "-x", "c", os.path.join(HERE, "flac_write", "fw_driver.c"), "-x", "none",
                               "-I" + os.path.join(MG.NQ, "third_party"), "-o", exe, nq_lib, "-lpthread", "-lm"])
        files = [(e[1]["name"], e[1]["rate"], e[1]["md5"], b, p) for e in es for b, p in e[0]]
        pack = os.path.join(tmp, "pack.bin")
        with open(pack, "wb") as f:
            f.write(struct.pack("<I", len(files)))
            for _, _, _, b, p in files:
                f.write(struct.pack("<QQ", len(b), p.size) + b + np.ascontiguousarray(p, "<i2").tobytes())
        run = subprocess.run([exe, pack], stdout=subprocess.PIPE, universal_newlines=True)
        lines = run.stdout.split("\n")[:-1]
        failed = [(files[i][:3], line) for i, line in enumerate(lines) if not line.endswith(" ok")]
        print("%d files through libFLAC, %d failed" % (len(lines), len(failed)))
    assert run.returncode == 0 and len(lines) == len(files) and not failed, (run.returncode, failed)
    json.dump(dict(cases=[e[1] for e in es]), open(os.path.join(HERE, "flac_write_any_golden.json"), "w"), indent=0)


if __name__ == "__main__":
    sys.exit(main())
