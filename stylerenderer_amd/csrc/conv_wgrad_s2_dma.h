// Internal interface of the LDS-DMA form of the stride-2 3x3 weight gradient (csrc/conv_wgrad_s2_dma.hip): the direct
// kernel's tiling, slices, partial slabs and result bits (csrc/conv_wgrad_mfma.hip), so it sizes, fills its kernel
// argument and reduces as the direct path does.
#pragma once
#include "conv_wgrad_mfma.h"

// 3x3 stride 2 on the direct plan's 16 x 4 patches: GW % 16 == 0, GH % 4 == 0, CU % 32 == 0, CV % 128 == 0, windows
// inside U, byte offsets < 2^31, SR_WGRAD_DMA != 0
bool sr_wgrad_s2_dma_eligible(const SrWgradTiles& t, int64_t B, int CU, int CV, int UH, int UW, int GH, int GW, int d0);
// launches nothing when p.B == 0
int sr_wgrad_s2_dma_launch(const WgradParams& p, const SrWgradTiles& t, hipStream_t st);
