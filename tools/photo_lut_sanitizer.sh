#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the arithmetic of the photometric stage that works on a value, an operation or a histogram alone
# (libheif_amd/csrc/photo_lut.h: the contrast mean, the autocontrast and equalize tables, BLEND, the point operations, the refusals), as a STAND-ALONE
# program with its own main (tests/emu/photo_lut_asan.cc; without arguments it runs its self-check).  CPU only; a few seconds.
# tests/test_photo_lut_host.py builds the same program and compares what it computes with tests/photo_ref.py.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${OUT_DIR:-$ROOT/build}/photo_lut_asan"
mkdir -p "$(dirname "$OUT")"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wextra -I"$ROOT/libheif_amd/csrc" \
    "$ROOT/tests/emu/photo_lut_asan.cc" -o "$OUT"
"$OUT"
