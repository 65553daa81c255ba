#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host code that builds the coefficient tables of HIPDEC_SCALE_BILINEAR / _BICUBIC
# (color.hip: hipdec_resample_taps and what it calls), as a STAND-ALONE program with its own main (tests/emu/resample_taps_asan.cc): every output index
# of the axes of tests/test_resample_ref.py, with exact and short capacities.  CPU only; takes about two minutes, nearly all of it the build.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${OUT_DIR:-$ROOT/build}/resample_taps_asan"
mkdir -p "$(dirname "$OUT")"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Wno-unknown-pragmas -fno-strict-aliasing -DHIPDEC_HOST_EMU=1 \
    -I"$ROOT/tests/emu/shim" -I"$ROOT/tests/emu" -I"$ROOT/include" -I"$ROOT/libheif_amd/csrc" \
    "$ROOT/tests/emu/resample_taps_asan.cc" -x c++ "$ROOT/libheif_amd/csrc/color.hip" -lpthread -o "$OUT"
"$OUT"
