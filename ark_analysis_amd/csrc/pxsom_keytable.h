// pxsom_keytable.h -- the key table of the cell-mask and cell-table kernels (K10, K12): int32 label -> its index in the
// sorted keys, by a dense LUT where one fits and a binary search where not.
//
// Everything on the device side is `static` (an unnamed namespace): a unit that includes this header gets its own
// lut_scatter_kernel.  The units are linked without relocatable device code, so a kernel has to be defined in the unit
// that launches it, and a unit emits the kernel whether it launches it or not -- which is why this is not part of
// pxsom_plane.h, which the units without a key table include too.  KeyTable keeps the mangled name it had when
// pxsom_cellquant.hip declared it, so the names of the kernels that take one stay what the profiles record.
#pragma once
#include "pxsom_plane.h"

namespace pxsom {

// The dense LUT of a key table: bytes of one int32 slot per value of [key_min, key_max], or 0 for the binary search --
// no keys, more than 64 MB of LUT, or a LUT far sparser than the table (over 16 slots a key + 64 Ki).
inline size_t dense_lut_bytes(int64_t n_keys, int32_t key_min, int32_t key_max)
{
    if (n_keys <= 0 || key_max < key_min) return 0;
    const int64_t range = (int64_t)key_max - key_min + 1;
    if (range > (int64_t(1) << 24) || range > 16 * n_keys + 65536) return 0;
    return (size_t)range * sizeof(int32_t);
}

}  // namespace pxsom

namespace {

struct KeyTable {
    const int32_t *keys;
    const int32_t *lut;        // dense route: index of key_min + i in keys, -1 when absent; nullptr: binary search
    int64_t n_keys;
    int32_t key_min;
    int64_t lut_size;
};

// index of `key` in t.keys, -1 when absent
__device__ __forceinline__ int64_t find_key(const KeyTable &t, int32_t key)
{
    if (t.lut) {
        const int64_t d = (int64_t)key - t.key_min;
        return d >= 0 && d < t.lut_size ? t.lut[d] : -1;
    }
    int64_t lo = 0, hi = t.n_keys;                    // first key >= `key`
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (t.keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < t.n_keys && t.keys[lo] == key ? lo : -1;
}

__global__ __launch_bounds__(256) void lut_scatter_kernel(const int32_t *__restrict__ keys, int64_t n, int32_t key_min,
                                                          int64_t lut_size, int32_t *__restrict__ lut)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t d = (int64_t)keys[i] - key_min;
        if (d >= 0 && d < lut_size) lut[d] = (int32_t)i;
    }
}

// fills the `bytes` (dense_lut_bytes) of `lut` on the stream and points `t` at it
inline int build_lut(KeyTable &t, int32_t *lut, size_t bytes, hipStream_t st)
{
    t.lut = lut;
    t.lut_size = (int64_t)(bytes / sizeof(int32_t));
    PXSOM_HIP_TRY(hipMemsetAsync(lut, 0xFF, bytes, st));   // every slot -1: absent
    hipLaunchKernelGGL(lut_scatter_kernel, dim3((unsigned)pxsom::flat_grid(t.n_keys, 4)), dim3(256), 0, st, t.keys, t.n_keys,
                       t.key_min, t.lut_size, lut);
    PXSOM_LAUNCH_CHECK("lut_scatter_kernel");
    return PXSOM_OK;
}

}  // namespace
