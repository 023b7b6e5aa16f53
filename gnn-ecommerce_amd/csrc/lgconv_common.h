// lgconv_common.h -- what the translation units of liblgconv_hip.so share (internal; the C ABI is include/lgconv_hip.h,
// which also carries the LGC_E_* codes and LGC_ST_* status bits).  Nothing lives here that only one unit uses.
//   host    ceil_div, as_stream, aligned_to, allow_big_lds / allow_lds
//   device  the contracts several entry points pin bit for bit, ONE definition each: the total order of lgc_mask_topk
//           (order_key, key_value), the guarded row loads (load4, load4_if), the four-step group of lgc_score_rows' chain
//           (score_chain), the sampler's stream (mix64, bounded), the search in a sorted list (lower_bound, in_sorted),
//           the wavefront reductions (wave_sum, wave_max, wave_or)
// The 64 x 128 x 32 fp32-MFMA tile of the scoring units is lgconv_tile.h, the selection two of them share is
// lgconv_select.h.  A helper moves here when a SECOND unit needs it, under an unprefixed name, and its copy in the first
// unit goes; a unit never restates one of these.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>

#include "lgconv_hip.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;  // 4 wavefronts, one per SIMD of a CU

typedef unsigned long long u64;
typedef float f4 __attribute__((ext_vector_type(4)));
// Row slices are only dword-aligned in general (D = 90 -> 360-byte rows; the overlapping last lane):
// tell the compiler, it still emits global_load_dwordx4 (gfx950 allows dword-aligned wide accesses).
typedef f4 f4u __attribute__((aligned(4)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
inline bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }   // nullptr is aligned

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

// Before a launch with `lds` bytes of dynamic LDS: above `limit` the kernel needs the opt-in, asked for once up to `bytes`.
inline int allow_lds(const void *fn, size_t lds, size_t limit, int bytes, unsigned long long *done_mask) {
    return lds > limit ? allow_big_lds(fn, bytes, done_mask) : 0;
}

// ----------------------------------------------------------------------------------------
// The total order of lgc_mask_topk, which every ranking entry point shares: a larger key is a better value.  Ascending
// with the value.  Every NaN, whatever its sign bit and payload, takes the one top key 0xFFFFFFFF: torch.topk ranks NaN as
// the largest value, and the sign of the NaN a seen +-inf score turns into (inf * 0) is the hardware's choice.  -0 and +0
// share a key (the add of +0 turns -0 into +0: a seen item's 0 * score).  Equal keys are ordered by index ascending, so NaNs
// come first by index, then +inf, the finite values, then -inf, whose key 0x007FFFFF is the smallest a value has: 0 is free
// to mean "nothing".
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t order_key(float v) {
    const float w = __fadd_rn(v, 0.0f);
    const uint32_t u = __float_as_uint(w);
    const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return w != w ? 0xFFFFFFFFu : key;
}

// the value a key stands for: order_key's inverse up to its folds (the NaN key gives the positive quiet NaN 0x7FFFFFFF)
__device__ __forceinline__ float key_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// Four floats of a table row starting at column d (d % 4 == 0); columns >= dim read as 0 and are never touched (the row
// may end there: padding columns, the next row, or the end of the allocation): one 16-byte load that need only be dword-
// aligned where all four columns exist, up to three dwords in the row's last group.  VEC: the width is a multiple of 4 and
// every row starts on 16 bytes, one aligned 16-byte load.
template <bool VEC>
__device__ __forceinline__ f4 load4(const float *__restrict__ row, int d, int dim) {
    if (VEC) return *reinterpret_cast<const f4 *>(row + d);
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (d + 4 <= dim) {
        v = *reinterpret_cast<const f4u *>(row + d);
    } else {
        if (d + 0 < dim) v.x = row[d + 0];
        if (d + 1 < dim) v.y = row[d + 1];
        if (d + 2 < dim) v.z = row[d + 2];
    }
    return v;
}

// the same, and zeros without a read where `live` is false (`row` need not be an address then)
__device__ __forceinline__ f4 load4_if(const float *__restrict__ row, int d, int dim, bool live) {
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (live) v = load4<false>(row, d, dim);
    return v;
}

// One group of lgc_score_rows' chain: acc after the fused multiply-adds of columns 4 g .. 4 g + 3 in ascending order, `a`
// the user-side factor.  A dot product in that entry point's bits is this over g = 0 .. ceil(dim / 4) - 1 ascending from
// +0 with zeros past dim, and NO group more: fma(0, 0, -0) is +0, an extra step could change a sign.
__device__ __forceinline__ float score_chain(f4 a, f4 b, float acc) {
    acc = __fmaf_rn(a.x, b.x, acc);
    acc = __fmaf_rn(a.y, b.y, acc);
    acc = __fmaf_rn(a.z, b.z, acc);
    acc = __fmaf_rn(a.w, b.w, acc);
    return acc;
}

// The sampler's stream: the splitmix64 finaliser as a counter-based generator, draw(seed, step, sample, attempt) is
// stateless.  lgc_sample_triples (lgconv_serve.hip) and lgc_sample_hard_triples (lgconv_hardneg.hip) draw from it with the
// same constants, which is what makes a hard negative one of the sampler's own draws; tests/sampler_support.py restates it.
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// unbiased integer in [0, range): 64-bit multiply-high of a 64-bit draw (bias < range / 2^64)
__device__ __forceinline__ uint64_t bounded(uint64_t r, uint64_t range) { return __umul64hi(r, range); }

// The first position of the ascending a[b, e) whose element is not below x, e where there is none; never reads outside
// [b, e).  (hi is declared before lo: the two selects of a step then come out in the order the open-coded loops had.)
template <typename I, typename T>
__device__ __forceinline__ I lower_bound(const T *__restrict__ a, I b, I e, T x) {
    I hi = e, lo = b;
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// does the ascending list a[b, e) (a user's ignore or seen list) hold x
template <typename I, typename T>
__device__ __forceinline__ bool in_sorted(const T *__restrict__ a, I b, I e, T x) {
    const I lo = lower_bound(a, b, e, x);
    return lo < e && a[lo] == x;
}

// Reductions over the 64 lanes of a wavefront, the result in every lane.  wave_sum is for sums whose order does not show
// (integers); a float sum whose bits are pinned keeps its own loop with its order spelled out.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) {
        const u64 o = __shfl_xor(v, m, kWave);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) v |= __shfl_xor(v, off);
    return v;
}

}  // namespace
