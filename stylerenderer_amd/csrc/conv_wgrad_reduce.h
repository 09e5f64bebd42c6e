// Internal interface of the slice reduction of the weight gradient (csrc/conv_wgrad_reduce.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wgrad_params.h"

// Adds the `ks` slabs of partial[ks][nt][UP][VP] in slice order into out.dwt: element (t, u < CU, v < CV) in the layout
// of `out`.  ks == 0 writes zeros.
int sr_wgrad_reduce_launch(const WgradOut& out, const float* partial, int ks, int nt, int UP, int VP, int CU, int CV,
                           hipStream_t st);
