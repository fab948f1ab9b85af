#!/bin/bash
# Builds csrc/conv_route.cpp with -fsanitize=address,undefined, links it with the library's other (plain) host objects and a stand-alone
# program that walks its three tables with NULL blobs, and runs that program on the CPU.  Needs the library built (flownet2_amd/build/*.o).
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(dirname "$HERE")"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
OUT="$(mktemp -d)"
trap 'rm -rf "$OUT"' EXIT
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
(cd "$ROOT" && python -m flownet2_amd.build > /dev/null)
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  -x hip -c "$ROOT/flownet2_amd/csrc/conv_route.cpp" -o "$OUT/conv_route.o"
"$HIPCC" -std=c++17 $SAN -I"$ROOT/include" -c "$HERE/conv_route_host_check.cpp" -o "$OUT/main.o"
OTHERS=$(ls "$ROOT"/flownet2_amd/build/*.o | grep -v '/conv_route\.cpp\.o$')
"$HIPCC" --offload-arch=gfx950 $SAN "$OUT/conv_route.o" "$OUT/main.o" $OTHERS -lz -o "$OUT/conv_route_host_check"
"$OUT/conv_route_host_check"
