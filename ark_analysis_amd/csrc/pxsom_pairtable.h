// pxsom_pairtable.h -- the run-compressed pair table of K18 (pxsom_merge.hip) and K21 (pxsom_nucsplit.hip): an
// open-addressing table of 64-bit pair keys with an int32 pixel count each, which takes one insertion per RUN of a pair.
// (K18's insert_runs_kernel has 70 SGPRs with table_add for the 66 of the probe loop it once spelled out; its stage,
// pair_overlaps at 2048 x 2048, measured inside the earlier form's own run-to-run spread: profiles/plane_shared/README.md.)
//
// A "run" is a stretch of pixels of one pair inside one row and inside one aligned group of 64 pixels of the flat raster
// order (a wave's pixels): a pure function of the image.  A caller counts the runs first, sizes the table for them
// (pair_slots: a power of two, at least twice the capacity) and makes no insertion when the runs exceed the capacity, so
// the table is at most half full whatever the labels are and a probe always ends at a free slot.
//
// Everything here is `static` (an unnamed namespace), as in pxsom_plane.h: every unit that includes the header gets its
// own copy.
#pragma once
#include "pxsom_common.h"

namespace {

constexpr unsigned long long kEmpty = ~0ull;
constexpr int64_t kMaxPairCapacity = int64_t(1) << 27;     // 2^28 slots of 12 bytes: 3 GiB of workspace
constexpr int kRunSpan = 16 * 256;                         // pixels per workgroup of the run passes

__device__ __forceinline__ unsigned long long mix64(unsigned long long k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// adds a run of `run` pixels of the pair `key` (never kEmpty) to the table; *n_pairs counts the slots taken
__device__ __forceinline__ void table_add(unsigned long long *__restrict__ keys, int32_t *__restrict__ counts, int64_t slots,
                                          unsigned long long key, int run, int32_t *__restrict__ n_pairs)
{
    int64_t slot = (int64_t)(mix64(key) & (unsigned long long)(slots - 1));
    for (int64_t probe = 0; probe < slots; probe++) {      // (ends long before: the table is at most half full)
        const unsigned long long old = atomicCAS(keys + slot, kEmpty, key);
        if (old == kEmpty) atomicAdd(n_pairs, 1);
        if (old == kEmpty || old == key) {
            atomicAdd(counts + slot, run);
            break;
        }
        slot = (slot + 1) & (slots - 1);
    }
}

// slots of the table for `capacity` pairs: a power of two, at least twice the capacity
inline int64_t pair_slots(int64_t capacity)
{
    int64_t s = 64;
    while (s < 2 * capacity) s <<= 1;
    return s;
}

// bytes of the keys of `slots` slots, 256-aligned: the counts follow them
inline size_t pair_keys_bytes(int64_t slots) { return pxsom::align_up((size_t)slots * sizeof(unsigned long long), 256); }

// bytes of the keys and the counts of a table for `capacity` pairs
inline size_t pair_table_bytes(int64_t capacity)
{
    const int64_t slots = pair_slots(capacity);
    return pair_keys_bytes(slots) + pxsom::align_up((size_t)slots * sizeof(int32_t), 256);
}

// the counts of a table of `slots` slots whose keys start at `keys`
inline int32_t *pair_table_counts(unsigned long long *keys, int64_t slots)
{
    return reinterpret_cast<int32_t *>(reinterpret_cast<char *>(keys) + pair_keys_bytes(slots));
}

}  // namespace
