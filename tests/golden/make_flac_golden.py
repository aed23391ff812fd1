#!/usr/bin/env python3
"""Generates the FLAC fixtures of dcs_encode_files from the reference's own code (build container only; outputs are data):
  flac_golden.{json,npz}  every file of tests/flac_cases.py (cases(), then refused_cases()) written as case.flac and run
                          through the reference's DCSEncoder::EncodeFile, with make_encode_file_golden's build and driver
                          unchanged (encode_file/ef_driver.cpp linked with the vendored libnyquist, whose FlacDecoder runs the
                          vendored libFLAC, and libsamplerate with the library's default table in its best-quality slot), at
                          versions 0x9400 and 0x9302: NyquistIO::Load's result (its float bits for the short cases, the sha256
                          of all of them, its exception text, or the crash) and EncodeFile's stream (whole up to 4 096 bytes,
                          else its sha256) or error text, and the reports of the sanitizer build
The generator asserts that every file of cases() loads in the reference, encodes wherever its rate and length allow, and
has no sanitizer report: a failing case means the writer is wrong, never that the case is dropped.  What the reference does
with each refused case is recorded as it is (INTEGRATION.md "Encoding files", rules 20-25, quote it).
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import flac_cases as F                          # noqa: E402
import make_encode_file_golden as MG            # noqa: E402
from oracle import flacref                      # noqa: E402  (libnyquist's build: one recipe)

HERE = MG.HERE


def main():
    import dcsexplorer_amd as D
    coeffs, inc = D.resample_filter_default()
    cases = [(n, b, "valid") for n, b in F.cases()] + [(c[0], c[1], "refused") for c in F.refused_cases()]
    meta, arrays, failed = [], {}, []
    with tempfile.TemporaryDirectory() as tmp:
        nq_lib = flacref.build_libnyquist(MG.NQ, os.path.join(tmp, "nq"))
        plain = MG.build(tmp, nq_lib, coeffs, inc)
        san = MG.build(tmp, nq_lib, coeffs, inc, extra=["-fsanitize=bounds,shift,float-cast-overflow"])
        for name, data, kind in cases:
            path = os.path.join(tmp, "case.flac")           # NyquistIO picks its decoder by the extension
            open(path, "wb").write(data)
            entry = dict(name=name, kind=kind, file_sha256=hashlib.sha256(data).hexdigest(), runs=[])
            for fv, typ, sub in MG.VERSIONS:
                s = MG.run(san, path, tmp, fv, typ, sub)
                p = MG.run(plain, path, tmp, fv, typ, sub)
                text = lambda t: t.replace("case.wav", "case.flac") if t is not None else None
                rec = dict(version=fv, type=typ, subType=sub, rc=p["rc"], load=text(p["load"]), encode=text(p["encode"]),
                           ubsan=s["ubsan"], san_rc=s["rc"])
                if p["stream"] is not None:
                    rec["bytes"] = len(p["stream"])
                    rec["sha256"] = hashlib.sha256(p["stream"]).hexdigest()
                    if len(p["stream"]) <= MG.KEEP_STREAM:
                        arrays["%s/%x/stream" % (name, fv)] = np.frombuffer(p["stream"], np.uint8)
                if fv == 0x9400 and p["values"] is not None:
                    entry["n_values"] = len(p["values"]) // 4
                    entry["values_sha256"] = hashlib.sha256(p["values"]).hexdigest()
                    if entry["n_values"] <= MG.KEEP_VALUES:
                        arrays[name + "/values"] = np.frombuffer(p["values"], "<f4")
                entry["runs"].append(rec)
            meta.append(entry)
            print(name, [(r["load"], r["encode"], r["ubsan"], r["rc"]) for r in entry["runs"]])
            if kind == "valid":
                for r in entry["runs"]:
                    if not (r["rc"] == 0 and r["load"] is not None and r["load"].startswith("ok") and r["ubsan"] == []
                            and r["san_rc"] == 0 and r["encode"] is not None and r["encode"].startswith("ok")
                            and "values_sha256" in entry):
                        failed.append((name, r))
    assert not failed, failed                   # (no exclusions: a failing case means the writer is wrong)
    np.savez_compressed(os.path.join(HERE, "flac_golden.npz"), **arrays)
    json.dump(dict(cases=meta, keep_values=MG.KEEP_VALUES, keep_stream=MG.KEEP_STREAM), open(os.path.join(HERE, "flac_golden.json"), "w"),
              indent=0)


if __name__ == "__main__":
    sys.exit(main())
