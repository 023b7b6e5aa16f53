#!/bin/bash
# The host side of bought-together in csrc/lgconv_cooccur.hip (the argument checks of lgc_cooccur_topk and the workspace size
# function) under AddressSanitizer + UBSan, as a stand-alone program: the unit and tools/asan_cooccur_host.cpp are compiled
# with the sanitizers on the host side only and linked into one executable, which is then run.  CPU only, no GPU is touched:
# every call returns before its launch.
# Usage: bash tools/asan_cooccur_host.sh
set -e
cd "$(dirname "$0")/.."
out=${TMPDIR:-/tmp}/lgconv_asan_cooccur
mkdir -p "$out"
san="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
flags="-O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Iinclude -Ignn-ecommerce_amd/csrc -Wall -Wno-unused-result"
/opt/rocm/bin/hipcc $flags $san -c gnn-ecommerce_amd/csrc/lgconv_cooccur.hip -o "$out/lgconv_cooccur.o" &
/opt/rocm/bin/hipcc $flags $san -x hip -c tools/asan_cooccur_host.cpp -o "$out/asan_cooccur_host.o"
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=address,undefined "$out/lgconv_cooccur.o" "$out/asan_cooccur_host.o" -o "$out/asan_cooccur_host"
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$out/asan_cooccur_host"
