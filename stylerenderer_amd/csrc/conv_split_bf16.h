// The switch of the opt-in split-bf16 spike (SR_CONV_SPLIT_BF16), read by both dispatch files: forward
// (csrc/conv_dispatch.hip) and weight gradient (csrc/conv_wgrad_dispatch.hip).  Defined in csrc/conv_wgrad_bf16x3.hip.
#pragma once

// kind: 'w' 1x1 weight gradient, 'g' stride-2 3x3 weight gradient, 'c' stride-2 3x3 convolution, 't' its transposed form
bool sr_wgrad_bf16x3_enabled(char kind);
