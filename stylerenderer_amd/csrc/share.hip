// The shared identity of a multi-view fit (C ABI: sr_share_rows; definition: stylerenderer_amd/op/share.py, share_rows_).
// g [B, d] holds the B views' gradients of the coefficients; the leading k columns belong to one variable all views
// share, whose gradient is the sum over the views.
//
//   k_share_rows   one lane per column j < k.  It walks the B rows twice: s = ((g[0, j] + g[1, j]) + g[2, j]) + ... in
//                  row order, then g[b, j] = s for every b.  A column is read and written by its own lane only, so the
//                  update is in place; neighbouring lanes touch neighbouring columns of a row (coalesced).
//
// One float32 addition per step in the definition's order (compiled with -ffp-contract=off; there is nothing to contract):
// the result is the host's bit for bit.  Vector stores and plain C++ only: no atomics, no LDS, no scratch, no memset, no
// host read, so it runs under graph capture on the caller's stream.
#include "common.h"

namespace {

constexpr int SH_BLOCK = 256;

__global__ __launch_bounds__(SH_BLOCK) void k_share_rows(float* __restrict__ g, int B, int64_t d, int64_t k) {
    const int64_t j = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
    if (j >= k) return;
    float s = g[j];
    for (int b = 1; b < B; ++b) s = s + g[(int64_t)b * d + j];
    for (int b = 0; b < B; ++b) g[(int64_t)b * d + j] = s;
}

}  // namespace

extern "C" int sr_share_rows(float* g, int64_t B, int64_t d, int64_t k, sr_stream_t stream) {
    if (B < 1 || d < 1 || k < 1 || k > d) return SR_EINVAL;
    if (!g) return SR_EINVAL;
    if (B > 65535 || d > (1LL << 31)) return SR_ERANGE;
    hipLaunchKernelGGL(k_share_rows, dim3((unsigned)sr_ceil_div(k, SH_BLOCK)), dim3(SH_BLOCK), 0, sr_stream(stream), g,
                       (int)B, d, k);
    return sr_launch_status();
}
