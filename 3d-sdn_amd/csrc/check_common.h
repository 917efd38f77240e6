// What the *_check.h headers share: the host/device qualifier of their index arithmetic, the failure macro of their validators,
// the pointer alignment test and the rounding of the workspace layouts.  Plain C++17, no HIP include: the tools/*_check.cpp
// programs build it with a host compiler alone.  (Device helpers live in device_common.h, which no *_check.h includes.)
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#if defined(__HIPCC__)
#define SDN_HD __host__ __device__ __forceinline__
#else
#define SDN_HD inline
#endif

// inside a validator `int f(..., char* msg, size_t cap)`: the reason into msg, 1 to the caller
#define SDN_FAIL(...)                         \
    do {                                      \
        std::snprintf(msg, cap, __VA_ARGS__); \
        return 1;                             \
    } while (0)

namespace sdn {

// `a` is a power of two
inline bool misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

inline size_t round_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

}  // namespace sdn
