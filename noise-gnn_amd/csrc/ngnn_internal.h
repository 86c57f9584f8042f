// Internal helpers shared by the ngnn HIP translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "ngnn.h"

#define NGNN_RETURN_IF(cond, code) \
    do {                           \
        if (cond) return (code);   \
    } while (0)

namespace ngnn {

constexpr int kWave = 64;  // CDNA wavefront

inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NGNN_OK : static_cast<int>(e);
}

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

inline bool fits_i32(int64_t v) { return v >= 0 && v <= INT32_MAX; }

inline bool aligned(const void *p, size_t a) {
    return (reinterpret_cast<uintptr_t>(p) % a) == 0;
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// a dropout probability outside [0, 1] (NaN included)
inline bool bad_p(float p) { return !(p >= 0.0f && p <= 1.0f); }

// Largest whole-buffer range in bytes: the kernels address a whole operand
// through one buffer resource with unsigned 32-bit offsets, and offsets from
// 0xF0000000 up mean "out of range" (kOOB) -- every such operand stays 4 KiB
// under that.
constexpr int64_t kRangeMax = 0xF0000000ll - 4096;

int num_cus();  // compute units of the current device (cached; ngnn_sage_rt.hip)

// Environment switches, for `static const` initialisers (read once per
// process): on unless the variable starts with '0'; an int, dflt when unset.
inline bool env_not_zero(const char *name) {
    const char *e = std::getenv(name);
    return !(e && e[0] == '0');
}
inline int env_int(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

// Runtime int -> template argument: f(std::integral_constant<int, V>{}) for
// the first V of the list equal to v; the last V is the default, as a
// switch ladder's `default:`.  (bools: with_const<1, 0>(flag, ...))
template <int V, int... Rest, class F>
inline void with_const(int v, F &&f) {
    if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>{});
    else if (v == V) f(std::integral_constant<int, V>{});
    else with_const<Rest...>(v, f);
}

// Raises kernel Kern's dynamic-LDS limit to `bytes`, once per instantiation
// (so once per kernel) and process.
template <auto Kern>
inline void max_dynamic_lds_once(size_t bytes) {
    static const hipError_t set = hipFuncSetAttribute(
        reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
    (void)set;
}

// The graph slot's contract gate (ABI 20): the slot kernel keeps, in a
// 64-bit word, (gen << 32 | bad bits) of the last load that broke the
// block's contract (atomicMax: the newest generation wins); gen_word is the
// slot's r_next word, whose high half is the current load's generation.  A
// step whose block broke the contract leaves the parameters and the step
// count untouched.  gate NULL: never gated.
__device__ __forceinline__ bool slot_gated(const uint64_t *gate, const int64_t *gen_word) {
    if (!gate || !gen_word) return false;
    const uint64_t g = *gate;
    return (g & 0xffffffffull) != 0 && (g >> 32) == (static_cast<uint64_t>(*gen_word) >> 32);
}

}  // namespace ngnn
