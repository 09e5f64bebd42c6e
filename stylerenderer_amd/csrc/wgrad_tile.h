// Scaffolding the K-sliced weight-gradient kernels share (k_wgrad_mfma, k_wgrad_s2_dma, k_wgrad_s2p, k_wgrad1_bf16x3,
// k_wgrad_s2_bf16x3): the workgroup's channel tile and K slice, the patch order of the three that walk patches, and
// the U window k_wgrad_s2_dma and k_wgrad_s2p stage with the same DMA instruction.  Under mfma_tile.h's rule: a helper
// keeps the expressions in the order the kernels had them written out, and a kernel adopts one only if its device code
// stays identical (scripts/compare_device_code.py --union; DESIGN.md 4.0 says what stayed private and why).
#pragma once
#include "mfma_tile.h"

// Workgroup bid of tiles_u * tiles_v * ks: the channel tiles of one K slice are neighbours, V tiles innermost.
struct SrWgradTile {
    int slice, u0, v0;
};
__host__ __device__ __forceinline__ constexpr SrWgradTile sr_wgrad_tile(int bid, int tiles_u, int tiles_v, int UT, int VT) {
    const int tile_uv = bid % (tiles_u * tiles_v);
    const int slice = bid / (tiles_u * tiles_v);
    return SrWgradTile{slice, (tile_uv / tiles_v) * UT, (tile_uv % tiles_v) * VT};
}

// patch = (b * tiles_y + ty) * tiles_x + tx: the patch order of the direct plan (sr_wgrad_tiles)
struct SrWgradPatch {
    int tx, ty, b;
};
__host__ __device__ __forceinline__ constexpr SrWgradPatch sr_wgrad_patch(int patch, int tiles_x, int tiles_y) {
    return SrWgradPatch{patch % tiles_x, (patch / tiles_x) % tiles_y, patch / (tiles_x * tiles_y)};
}

// The U window of a row group of a 16 x 4 stride-2 patch (16 x 2 grid positions x 3 x 3 taps = 5 rows x 33 columns) as
// k_wgrad_s2_dma and k_wgrad_s2p stage it: ONE 16-byte LDS-DMA instruction of 45 lanes = 5 rows x 9 float4 per
// channel, 32 channels at an odd pitch (the 32 lanes of an operand fetch hit 32 banks), two such blocks in front of V.
namespace sr_s2_window {
constexpr int ROWS = 5, QUADS = 9, LANES = ROWS * QUADS;      // 45 lanes fetch
constexpr int RP = 4 * QUADS;                                 // 36 floats per staged window row (33 used)
constexpr int UPL = ROWS * RP + 1;                            // 181: channel pitch
constexpr int BLOCK = 32 * UPL;                               // 5792 floats: one row group of the 32 U channels
constexpr int OFF_V = 2 * BLOCK;                              // 11584: V behind two blocks
// byte offset of lane's float4 from the window's first float in a U plane of row pitch UW
__host__ __device__ __forceinline__ constexpr int lane_off(int lane, int UW) { return ((lane / QUADS) * UW + 4 * (lane % QUADS)) * 4; }
}  // namespace sr_s2_window

namespace sr_wgrad_tile_checks {
// every (slice, u tile, v tile) exactly once, in the order the header states
constexpr bool tile_decode_enumerates(int tiles_u, int tiles_v, int ks, int UT, int VT) {
    int bid = 0;
    for (int s = 0; s < ks; ++s)
        for (int u = 0; u < tiles_u; ++u)
            for (int v = 0; v < tiles_v; ++v, ++bid) {
                const SrWgradTile t = sr_wgrad_tile(bid, tiles_u, tiles_v, UT, VT);
                if (t.slice != s || t.u0 != u * UT || t.v0 != v * VT) return false;
            }
    return true;
}
constexpr bool patch_decode_enumerates(int tiles_x, int tiles_y, int tiles_b) {
    int patch = 0;
    for (int b = 0; b < tiles_b; ++b)
        for (int y = 0; y < tiles_y; ++y)
            for (int x = 0; x < tiles_x; ++x, ++patch) {
                const SrWgradPatch t = sr_wgrad_patch(patch, tiles_x, tiles_y);
                if (t.tx != x || t.ty != y || t.b != b) return false;
            }
    return true;
}
static_assert(tile_decode_enumerates(3, 2, 4, 32, 128) && tile_decode_enumerates(1, 5, 2, 64, 64), "sr_wgrad_tile");
static_assert(patch_decode_enumerates(4, 3, 2) && patch_decode_enumerates(1, 8, 3), "sr_wgrad_patch");
static_assert(sr_s2_window::RP >= 2 * 16 + 1 && sr_s2_window::UPL % 2 == 1, "33 used columns per row, odd channel pitch");
static_assert(sr_s2_window::lane_off(0, 65) == 0 && sr_s2_window::lane_off(8, 65) == 32 * 4 &&
                  sr_s2_window::lane_off(9, 65) == 65 * 4 && sr_s2_window::lane_off(sr_s2_window::LANES - 1, 65) == (4 * 65 + 32) * 4,
              "lane = row * 9 + float4 of the row");
}  // namespace sr_wgrad_tile_checks
