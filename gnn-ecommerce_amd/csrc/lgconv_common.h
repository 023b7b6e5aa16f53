// lgconv_common.h -- what the translation units of liblgconv_hip.so share (internal; the C ABI is include/lgconv_hip.h,
// which also carries the LGC_E_* codes and LGC_ST_* status bits).  Nothing lives here that only one unit uses.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>

#include "lgconv_hip.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;  // 4 wavefronts, one per SIMD of a CU

typedef float f4 __attribute__((ext_vector_type(4)));
// Row slices are only dword-aligned in general (D = 90 -> 360-byte rows; the overlapping last lane):
// tell the compiler, it still emits global_load_dwordx4 (gfx950 allows dword-aligned wide accesses).
typedef f4 f4u __attribute__((aligned(4)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// The opt-in for more than 64 KiB of dynamic LDS is per DEVICE: remember it per device ordinal.
inline int allow_big_lds(const void *fn, int bytes, unsigned long long *done_mask) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev >= 0 && ((*done_mask >> dev) & 1ull)) return 0;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    if (dev >= 0) *done_mask |= 1ull << dev;
    return 0;
}

}  // namespace
