#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host code of the warp stage that works on a map alone (libheif_amd/csrc/warp_host.h: the refusals,
# Pillow's fixed-point values, the running-sum index tables of its scale path), as a STAND-ALONE program with its own main
# (tests/emu/warp_tables_asan.cc).  CPU only; a few seconds.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${OUT_DIR:-$ROOT/build}/warp_tables_asan"
mkdir -p "$(dirname "$OUT")"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wextra -I"$ROOT/libheif_amd/csrc" \
    "$ROOT/tests/emu/warp_tables_asan.cc" -o "$OUT"
"$OUT"
