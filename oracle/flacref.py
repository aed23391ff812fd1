#!/usr/bin/env python3
"""Builds the vendored libnyquist (whose FlacDecoder runs the vendored libFLAC), UNMODIFIED and where it lies under the
reference tree, as checker binaries for the FLAC reader and writer (test infrastructure):

  oracle/_ref/dcs_flacref       tests/golden/flac/flacref_driver.cpp: NyquistIO::Load over a pack of files, one child process a
                                file, and (mode md5) tests/golden/flac_write/fw_driver.c's FLAC__stream_decoder with MD5 checking
                                over (file, source PCM) pairs
  oracle/_ref/dcs_flacref_san   the same, libnyquist and libFLAC included, with -fsanitize=bounds,shift,float-cast-overflow (host
                                code): a file on which it reports is one where the reference's answer depends on its binary

libnyquist is built with its own CMake (-G Ninja, LIBNYQUIST_BUILD_EXAMPLE=OFF, whose example target has no sources) into
oracle/_ref/flacref_build/.  The golden generators make_encode_file_golden.py, make_flac_golden.py and
make_flac_write_golden.py build their archive with build_libnyquist() too: one recipe.

  python3 oracle/flacref.py <reference root> <output directory>
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BINARIES = ("dcs_flacref", "dcs_flacref_san")
SANITIZE = "-fsanitize=bounds,shift,float-cast-overflow"
JOBS = 16


def build_libnyquist(nq, build_dir, flags=()):
    """the vendored libnyquist at `nq` built into build_dir, every source compiled with `flags` as well -> the archive's path"""
    cmd = ["cmake", "-Wno-dev", "-G", "Ninja", "-S", nq, "-B", build_dir, "-DLIBNYQUIST_BUILD_EXAMPLE=OFF", "-DCMAKE_BUILD_TYPE=Release"]
    if flags:
        cmd += ["-DCMAKE_C_FLAGS=" + " ".join(flags), "-DCMAKE_CXX_FLAGS=" + " ".join(flags)]
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    subprocess.check_call(["ninja", "-C", build_dir, "-j%d" % JOBS], stdout=subprocess.DEVNULL)
    return os.path.join(build_dir, "lib", "liblibnyquist.a")


def build_checker(nq, work, exe, flags=()):
    os.makedirs(work, exist_ok=True)
    lib = build_libnyquist(nq, os.path.join(work, "nq"), flags)
    fw = os.path.join(work, "fw_driver.o")
    # (fw_driver.c keeps its own main for make_flac_write_golden.py; here it is the checker's md5 mode)
    subprocess.check_call(["gcc", "-O2", "-w", "-Dmain=fw_main", "-I" + os.path.join(nq, "third_party"), "-c",
                           os.path.join(GOLDEN, "flac_write", "fw_driver.c"), "-o", fw] + list(flags))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-I" + os.path.join(nq, "include"), "-o", exe,
                           os.path.join(GOLDEN, "flac", "flacref_driver.cpp"), fw] + list(flags)
                          + ["-Wl,--whole-archive", lib, "-Wl,--no-whole-archive", "-lpthread", "-lm"])
    return exe


def main(argv):
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    nq, out = os.path.join(argv[1], "libnyquist"), os.path.abspath(argv[2])
    work = os.path.join(out, "flacref_build")
    build_checker(nq, os.path.join(work, "plain"), os.path.join(out, BINARIES[0]))
    build_checker(nq, os.path.join(work, "san"), os.path.join(out, BINARIES[1]), flags=[SANITIZE])
    print("built oracle/_ref/%s from %s" % (", ".join(BINARIES), nq))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
