#!/bin/bash
# The host side of cross-table retrieval in csrc/lgconv_retrieve.hip (the argument checks of lgc_retrieve_topk and the
# workspace size function) under AddressSanitizer + UBSan, as a stand-alone program: the unit and tools/asan_retrieve_host.cpp
# are compiled with the sanitizers on the host side only and linked into one executable, which is then run
# (csrc/lgconv_hip.hip comes along for lgc_dim_ok).  CPU only, no GPU is touched: every call returns before its launch.
# Usage: bash tools/asan_retrieve_host.sh
set -e
cd "$(dirname "$0")/.."
out=${TMPDIR:-/tmp}/lgconv_asan_retrieve
mkdir -p "$out"
san="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
flags="-O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Iinclude -Ignn-ecommerce_amd/csrc -Wall -Wno-unused-result"
for unit in lgconv_retrieve lgconv_hip; do
    /opt/rocm/bin/hipcc $flags $san -c gnn-ecommerce_amd/csrc/$unit.hip -o "$out/$unit.o" &
done
wait
/opt/rocm/bin/hipcc $flags $san -x hip -c tools/asan_retrieve_host.cpp -o "$out/asan_retrieve_host.o"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=address,undefined "$out/lgconv_retrieve.o" "$out/lgconv_hip.o" "$out/asan_retrieve_host.o" -o "$out/asan_retrieve_host"
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$out/asan_retrieve_host"
