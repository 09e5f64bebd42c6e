// Kernel argument of the direct and the fused dense-convolution kernels (csrc/conv_mfma.hip, csrc/convt_fused.hip)
// and of their reduce kernels: passed by value, so its layout IS their kernarg segment.  csrc/conv_dispatch.hip fills
// the call's part (buffers, extents, scratch); each launcher sets the geometry of its own launches.
#pragma once
#include <stdint.h>

struct ConvParams {
    const float* in;
    const float* wt;
    const float* iscale;
    const float* oscale;
    const float* obias;
    float* out;
    int B, C, N, ldw;    // ldw: row pitch of wt in floats (multiple of 4, >= N)
    int IH, IW;          // input extent
    int GH, GW;          // output grid (phase space): rows [gy_base, GH), columns [gx_base, GW)
    int gy_base, gx_base;
    int OH, OW;          // full output extent
    int osy, osx, ooy, oox;   // output coordinate = grid * os + oo
    int dy0, dx0;        // input coordinate = grid * IS + d0 + tap
    int wmap[9];         // weight slab of window position (ty, tx)
    int tiles_x, tiles_y, tiles_b, tiles_n;
    // split-K for small feature maps (few tiles, long serial K loop): slice s handles channels
    // [s * c_per_slice, (s+1) * c_per_slice) and writes raw sums to partial[s] (layout of `out`);
    // k_conv_reduce adds the slices in order and applies oscale / bias.  ks == 1: direct epilogue.
    float* partial;
    int64_t partial_floats;
    int ks, c_per_slice;
    // TAP9 launches: the taps this launch walks are tap_first + i * tap_step, i < tap_count (all nine: 0, 1, 9; the
    // border strips behind the fused kernel: row 2*IH = taps 6, 7, 8; column 2*IW = taps 2, 5, 8)
    int tap_first, tap_step, tap_count;
};
