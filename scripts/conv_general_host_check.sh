#!/bin/bash
# Builds the host side of the general convolution with -fsanitize=address,undefined into a stand-alone program and runs it on the CPU.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(dirname "$HERE")"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
OUT="$(mktemp -d)"
trap 'rm -rf "$OUT"' EXIT
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  -I"$ROOT/include" -x hip -c "$ROOT/flownet2_amd/csrc/conv_general.hip" -o "$OUT/conv_general.o"
"$HIPCC" -std=c++17 $SAN -I"$ROOT/include" -c "$HERE/conv_general_host_check.cpp" -o "$OUT/main.o"
"$HIPCC" $SAN "$OUT/conv_general.o" "$OUT/main.o" -o "$OUT/conv_general_host_check"
"$OUT/conv_general_host_check"
