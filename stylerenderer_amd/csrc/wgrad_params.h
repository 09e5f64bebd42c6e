// Kernel argument of the direct weight-gradient kernels (k_wgrad_mfma of csrc/conv_wgrad_mfma.hip, k_wgrad_s2_dma of
// csrc/conv_wgrad_s2_dma.hip): passed by value, so its layout IS their kernarg segment.  And the output layout every
// path's last kernel (a reduce or a finish) writes, which csrc/conv_wgrad_dispatch.hip works out once per call.
#pragma once
#include <stdint.h>

struct WgradParams {
    const float* U;
    const float* V;
    const float* uscale;
    const float* vscale;
    float* partial;       // [KS][NT][UP][VP]
    int B, CU, CV;        // channels of U and V
    int UH, UW;           // extent of U
    int GH, GW;           // base grid (= extent of V)
    int dy0, dx0;         // U coordinate = grid * IS + d0 + tap
    int tiles_x, tiles_y, tiles_b;    // patches
    int tiles_u, tiles_v;
    int ks, patches_per_slice;
    int UP, VP;           // padded channel extents (tiles_u * UT, tiles_v * VT)
};

// Element (tap t, U channel u, V channel v) goes to dwt[t * slab + u * su + v * sv]: dwt is [taps][C][N], and a regular
// convolution has (u, v) = (c, n), the transposed one (u, v) = (n, c).
struct WgradOut {
    float* dwt;
    int64_t slab, su, sv;
};
