#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the arithmetic of the augment stage that works on a pixel, an operation or a radius alone
# (libheif_amd/csrc/augment_lut.h: Pillow's RGB <-> HSV conversions, the hue shift, the extended-box parameters of ImageFilter.GaussianBlur, one box pass
# over a line, the refusals), as a STAND-ALONE program with its own main (tests/emu/augment_lut_asan.cc; without arguments it runs its self-check).
# CPU only; a few seconds.  tests/test_augment_lut_host.py builds the same program and compares what it computes with tests/augment_ref.py.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${OUT_DIR:-$ROOT/build}/augment_lut_asan"
mkdir -p "$(dirname "$OUT")"
g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wextra -I"$ROOT/libheif_amd/csrc" \
    "$ROOT/tests/emu/augment_lut_asan.cc" -o "$OUT"
"$OUT"
