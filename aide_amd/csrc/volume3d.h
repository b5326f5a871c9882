// What the 3-D volume operators share (eval3d.hip, metrics_mc.hip, surface3d.hip, morph3d.hip): how a strided int64 / uint8
// volume is read on the device, and on the host the checks of its dims and spacing and the carving of a workspace.
#pragma once
#include "common.h"

#include <cmath>

// A strided operand: voxel (0, 0, 0) and the element strides of the logical dims; u8: bytes, otherwise int64
struct Operand {
    const void* p;
    long s0, s1, s2;
    int u8;
    __device__ __forceinline__ long off(int i0, int i1, int i2) const { return (long)i0 * s0 + (long)i1 * s1 + (long)i2 * s2; }
    // for kernels templated on the element type: no branch on u8
    template <typename T>
    __device__ __forceinline__ long long at(long o) const { return (long long)static_cast<const T*>(p)[o]; }
    __device__ __forceinline__ long long at(long o) const { return u8 ? at<unsigned char>(o) : at<long long>(o); }
};

// raster index -> logical index of a volume with the trailing dims (d1, d2)
__device__ __forceinline__ void raster_decode(int i, int d1, int d2, int& i0, int& i1, int& i2) {
    const int plane = d1 * d2;
    i0 = i / plane;
    const int r = i - i0 * plane;
    i1 = r / d2;
    i2 = r - i1 * d2;
}

// everything the grids and the raster indices need fits an int
static inline bool dims_ok(int64_t d0, int64_t d1, int64_t d2) {
    if (d0 < 0 || d1 < 0 || d2 < 0) return false;
    if (d0 == 0 || d1 == 0 || d2 == 0) return true;
    return d0 <= INT32_MAX && d1 <= INT32_MAX && d2 <= INT32_MAX && d1 * d2 <= INT32_MAX && d0 * (d1 * d2) <= INT32_MAX;
}

static inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// three finite positive spacings
static inline bool spacing_ok(const double* sp) {
    for (int k = 0; k < 3; ++k)
        if (!(sp[k] > 0.0) || !std::isfinite(sp[k])) return false;
    return true;
}

// A workspace handed out from the front, every piece rounded up to 16 bytes.  ws = nullptr measures: a *_ws_bytes entry and its
// launcher walk the same sequence of take() calls, so the layout is stated once.
struct Carver {
    char* at;
    size_t used = 0;
    explicit Carver(void* ws = nullptr) : at(static_cast<char*>(ws)) {}
    template <typename T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(at ? at + used : nullptr);
        used += align16(count * sizeof(T));
        return p;
    }
};
