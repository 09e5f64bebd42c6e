// Staging shared by the two interior kernels of the stride-2 transposed 3x3 convolution, k_convt_fused
// (csrc/convt_fused.hip) and k_convt_wino (csrc/convt_wino.hip): K chunks of CONVT_KC input channels, the raw halo
// patch [KC][PH + 1][36] and the raw taps [taps][KC][NB] moved by 16-byte buffer-addressed LDS-DMA.  A wave
// instruction moves 1 KiB = 256 floats; instruction j of a chunk belongs to wave j % 4, slot j / 4.  Lanes with
// nothing to fetch (outside the image: the in[-1] halo; surplus instructions) point beyond the buffer and receive
// zeros; a surplus instruction lands in the pad zone behind the two buffers.  The chunk part of every address is the
// scalar soffset of the buffer load: no vector ALU work per DMA instruction.
#pragma once
#include "mfma_tile.h"

constexpr int CONVT_KC = 8;                       // input channels per chunk = 4 k-steps
constexpr int CONVT_PW = 32;                      // input columns per workgroup
constexpr int CONVT_LEAD = 3;                     // halo columns start at i0 - 4 (aligned); i0 - 1 is column 3
constexpr int CONVT_EWP = CONVT_LEAD + 1 + CONVT_PW;   // 36

#if __HIP_DEVICE_COMPILE__
// Byte offsets inside one sample, chunk 0, of this lane's pieces of the halo patch: rows j0 - 1 .. of PLANE / 36 rows,
// columns i0 - 4 .. i0 + 31.
template <int PLANE, int I_INSTR, class P>
__device__ __forceinline__ int convt_patch_offset(const P& p, int j, int lane, int j0, int i0) {
    static_assert(PLANE % 4 == 0 && CONVT_EWP % 4 == 0, "16-byte DMA pieces must not straddle a row");
    const int f = (j * 64 + lane) * 4;
    int off = SR_BUF_OOB;
    if (j < I_INSTR && f < CONVT_KC * PLANE) {
        const int c = f / PLANE, q = f % PLANE;
        const int r = q / CONVT_EWP, cola = q % CONVT_EWP;
        const int gy = j0 - 1 + r, gx = i0 - 4 + cola;
        if (gy >= 0 && gy < p.IH && gx >= 0 && (gx | 3) < p.IW) off = ((c * p.IH + gy) * p.IW + gx) * 4;
    }
    return off;
}
#endif
