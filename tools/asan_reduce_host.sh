#!/bin/bash
# The host builder of the concatenated operator in csrc/lgconv_reduce.hip (lgc_reduce_concat_host, and the argument checks
# of lgc_reduce_concat) under AddressSanitizer + UBSan, as a stand-alone program: the unit and tools/asan_reduce_host.cpp
# are compiled with the sanitizers on the host side only and linked into one executable, which is then run.
# CPU only, no GPU is touched: the device entry point is only given arguments it rejects before its first launch.
# Usage: bash tools/asan_reduce_host.sh
set -e
cd "$(dirname "$0")/.."
out=${TMPDIR:-/tmp}/lgconv_asan_reduce
mkdir -p "$out"
san="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
flags="-O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Iinclude -Ignn-ecommerce_amd/csrc -Wall -Wno-unused-result"
/opt/rocm/bin/hipcc $flags $san -c gnn-ecommerce_amd/csrc/lgconv_reduce.hip -o "$out/lgconv_reduce.o" &
/opt/rocm/bin/hipcc $flags $san -x hip -c tools/asan_reduce_host.cpp -o "$out/asan_reduce_host.o"
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=address,undefined "$out/lgconv_reduce.o" "$out/asan_reduce_host.o" -o "$out/asan_reduce_host"
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$out/asan_reduce_host"
