// Scaffolding the LDS-DMA / MFMA kernels share: operand and pointer types, the workgroup renumbering, the tile decode,
// the 32x32 MFMA C/D layout and the host-side opt-in to large dynamic LDS.  Every device helper
// is __forceinline__ and keeps its expressions in the order the kernels had them written out: adopting one must not
// change a kernel's device code (scripts/compare_device_code.py --union is the check).
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef const void __attribute__((address_space(1)))* gptr_t;
typedef void __attribute__((address_space(3)))* lptr_t;

// Byte offset beyond every buffer resource: a buffer load (LDS-DMA included) from it returns zeros.  Lanes with
// nothing to fetch use it, so every lane issues every DMA.
constexpr int SR_BUF_OOB = 0x7FFFFFF0;

// Workgroup renumbering.  Hardware workgroup id `bid` of `nwg` runs on XCD bid % 8; the result numbers the workgroups
// of one XCD consecutively (chunks of nwg / 8, the first nwg % 8 chunks one longer), so that neighbours in the
// kernel's own tile order — which share input patches and weights — share that XCD's L2.
__host__ __device__ __forceinline__ constexpr int sr_xcd_chunk(int bid, int nwg) {
    const int q = nwg / SR_NUM_XCD, r = nwg % SR_NUM_XCD, xcd = bid % SR_NUM_XCD;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / SR_NUM_XCD;
}

// id = ((rest * tiles_y + ty) * tiles_x + tx) * tiles_n + n_t: output-channel tiles of one patch are neighbours
struct SrTile {
    int n_t, tx, ty, rest;
};
__device__ __forceinline__ SrTile sr_tile_decode(int id, int tiles_n, int tiles_x, int tiles_y) {
    SrTile t;
    t.n_t = id % tiles_n;
    id /= tiles_n;
    t.tx = id % tiles_x;
    id /= tiles_x;
    t.ty = id % tiles_y;
    t.rest = id / tiles_y;
    return t;
}

// C/D layout of v_mfma_f32_32x32x*: accumulator register r of a lane in half-wave `half` (lane >> 5) holds row
// sr_mfma32_row(r, half) of column lane & 31
__host__ __device__ __forceinline__ constexpr int sr_mfma32_row(int r, int half, int base = 0) {
    return base + (r & 3) + 8 * (r >> 2) + 4 * half;
}

namespace sr_tile_checks {
constexpr bool xcd_chunk_permutes(int nwg) {
    bool seen[40] = {};
    for (int bid = 0; bid < nwg; ++bid) {
        const int v = sr_xcd_chunk(bid, nwg);
        if (v < 0 || v >= nwg || seen[v]) return false;
        seen[v] = true;
    }
    return true;
}
constexpr bool xcd_chunk_permutes_upto(int n) {
    for (int nwg = 1; nwg <= n; ++nwg)
        if (!xcd_chunk_permutes(nwg)) return false;
    return true;
}
constexpr bool mfma32_rows_cover() {
    bool seen[32] = {};
    for (int half = 0; half < 2; ++half)
        for (int r = 0; r < 16; ++r) {
            const int v = sr_mfma32_row(r, half);
            if (v < 0 || v >= 32 || seen[v]) return false;
            seen[v] = true;
        }
    return true;
}
static_assert(xcd_chunk_permutes_upto(40), "sr_xcd_chunk(., nwg) is a permutation of 0 .. nwg - 1 (both sides of nwg % 8)");
static_assert(mfma32_rows_cover(), "sr_mfma32_row maps r = 0 .. 15, half = 0, 1 onto 0 .. 31 exactly once");
}  // namespace sr_tile_checks

// Opt-in to more than 64 KiB of dynamic LDS, once per kernel instantiation and process (never per launch).  False
// when the runtime refuses: the error is cleared and the caller returns SR_EINVAL without launching.
template <auto Kernel>
static inline bool sr_allow_dynamic_lds(int bytes) {
    static bool allowed = false;
    if (!allowed) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) !=
            hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        allowed = true;
    }
    return true;
}
