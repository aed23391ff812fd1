#!/usr/bin/env python3
"""Generates the FLAC writer's fixture (build container only; the output is data):
  flac_write_golden.json  per case of tests/flac_write_cases.py, with and without the MD5: the sha256 and the size of the
                          file tests/flac_write_ref.py writes and its counts of block kinds; for the many-stream shapes the
                          sha256 of the streams' concatenation, its size and the summed counts
Every file is first decoded by the vendored libFLAC: libnyquist is built as make_flac_golden.py builds it (in a temp dir),
and flac_write/fw_driver.c is linked against the archive's libFLAC and runs FLAC__stream_decoder over each file with MD5
checking on.  The generator asserts that libFLAC accepts every file, that the decoded samples equal the source and that
the MD5 check passes (for the files written without an MD5, libFLAC has nothing to compare and the first two hold).  There
are no exclusions: a failing case means the writer is wrong.
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

import flac_write_cases as C                    # noqa: E402
import flac_write_ref as R                      # noqa: E402
import make_encode_file_golden as MG            # noqa: E402
from oracle import flacref                      # noqa: E402  (libnyquist's build: one recipe)

HERE = MG.HERE
KINDS = ("nBlocks", "nConstant", "nVerbatim", "nFixed")


def entries():
    """-> [(name, md5, [(flac bytes, pcm)], record)]"""
    out = []
    for md5 in (True, False):
        for name, pcm in C.cases():
            b, info = R.write(pcm, 31250, md5)
            rec = dict(name=name, md5=md5, sha256=hashlib.sha256(b).hexdigest(), bytes=len(b), **{k: info[k] for k in KINDS})
            out.append((name, md5, [(b, pcm)], rec))
        for name, pool, index in C.shapes():
            written = [R.write(p, 31250, md5) for p in pool]
            h, size, kinds = hashlib.sha256(), 0, dict.fromkeys(KINDS, 0)
            for i in index:
                h.update(written[i][0])
                size += len(written[i][0])
                for k in KINDS:
                    kinds[k] += written[i][1][k]
            rec = dict(name=name, md5=md5, streams=len(index), sha256=h.hexdigest(), bytes=size, **kinds)
            out.append((name, md5, [(w[0], p) for w, p in zip(written, pool)], rec))        # (each distinct stream once)
    return out


def main():
    es = entries()
    with tempfile.TemporaryDirectory() as tmp:
        nq_lib = flacref.build_libnyquist(MG.NQ, os.path.join(tmp, "nq"))
        exe = os.path.join(tmp, "fw_driver")
        subprocess.check_call(["g++", "-O2", "-w", "-x", "c", os.path.join(HERE, "flac_write", "fw_driver.c"), "-x", "none",
                               "-I" + os.path.join(MG.NQ, "third_party"), "-o", exe, nq_lib, "-lpthread", "-lm"])
        files = [(e[0], e[1], b, p) for e in es for b, p in e[2]]
        pack = os.path.join(tmp, "pack.bin")
        with open(pack, "wb") as f:
            f.write(struct.pack("<I", len(files)))
            for _, _, b, p in files:
                f.write(struct.pack("<QQ", len(b), p.size) + b + np.ascontiguousarray(p, "<i2").tobytes())
        run = subprocess.run([exe, pack], stdout=subprocess.PIPE, universal_newlines=True)
        lines = run.stdout.split("\n")[:-1]
        failed = [(files[i][0], files[i][1], line) for i, line in enumerate(lines) if not line.endswith(" ok")]
        print("%d files through libFLAC, %d failed" % (len(lines), len(failed)))
    assert run.returncode == 0 and len(lines) == len(files) and not failed, (run.returncode, failed)
    json.dump(dict(cases=[e[3] for e in es]), open(os.path.join(HERE, "flac_write_golden.json"), "w"), indent=0)


if __name__ == "__main__":
    sys.exit(main())
