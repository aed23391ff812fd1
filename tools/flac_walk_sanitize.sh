#!/bin/bash
# tools/flac_walk_sanitize.sh -- the FLAC reader's host parse and the host instantiations of its walk, restore and mix
# (tests/cpp/dcs_flac_walk_san.cpp) under AddressSanitizer + UBSan, over every file the FLAC tests upload: flac_cases' accepted and
# refused cases and every well-formed and damaged file of tests/flac_fuzz_cases.py.  A stand-alone program, host code only
# (-Xarch_host; the device code is compiled untouched and never run): run it where it was built, never on a GPU machine, and
# before a new seed's damaged files go to one.  It also compares status, frame and code of every file with what
# tests/flac_ref.py predicts.  Needs libdcs_hip.so built (the program's other host symbols come from it).
#   tools/flac_walk_sanitize.sh [work directory, default a fresh temporary one]
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$(mktemp -d)}; mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
${PYTHON:-python3} "$ROOT/tests/flac_fuzz_cases.py" --pack "$OUT/flac_walk.pack"
$HIPCC -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -w -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  -Xarch_host -fno-omit-frame-pointer -c "$ROOT/tests/cpp/dcs_flac_walk_san.cpp" -o "$OUT/dcs_flac_walk_san.o"
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize -o "$OUT/dcs_flac_walk_san" "$OUT/dcs_flac_walk_san.o" \
  -L"$ROOT/dcsexplorer_amd" -ldcs_hip -Wl,-rpath,"$ROOT/dcsexplorer_amd"
ASAN_OPTIONS=detect_leaks=1 "$OUT/dcs_flac_walk_san" "$OUT/flac_walk.pack" > "$OUT/flac_walk.out"
cut -d' ' -f1-3 "$OUT/flac_walk.out" | diff - "$OUT/flac_walk.pack.expect" > "$OUT/flac_walk.diff" \
  || { echo "the host walk and tests/flac_ref.py differ: $OUT/flac_walk.diff"; head "$OUT/flac_walk.diff"; exit 1; }
echo "clean: $(wc -l < "$OUT/flac_walk.out") files, no sanitizer report, every status, frame and code as tests/flac_ref.py predicts"
