// The adjoint of the corner explode of op.texture.uv_map (C ABI: sr_explode_bwd; definition: stylerenderer_amd/op/texture.py,
// explode).  The uv map draws the mesh with its corners exploded, c[b, 3 f + k] = v[b, tri[f, k]], so the gradient of a
// vertex is the sum of its corners' gradients.  A library's index_put(accumulate=True) sorts the 3 nf constant indices in
// every call; here a lane owns one vertex of one sample and adds its corners in the fixed order of the topology's
// incidence list (op.rasterize.incidence: off int32 [nv + 2], adj int32 [3 nf], the entries k nf + f of a vertex
// ascending), each coordinate from 0.  One launch, no atomics, no scratch, no host read: it runs under graph capture and
// reruns are bit-identical.  A vertex no face uses gets exactly 0.
#include "common.h"

namespace {

constexpr int EX_BLOCK = 256;

__global__ __launch_bounds__(EX_BLOCK) void k_explode_bwd(float* __restrict__ gv, const float* __restrict__ gc,
                                                          const int32_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                          int64_t B, int64_t nv, int64_t nf) {
    const int64_t item = (int64_t)blockIdx.x * EX_BLOCK + threadIdx.x;
    if (item >= B * nv) return;
    const int64_t b = item / nv, i = item % nv, n_adj = 3 * nf;
    // a list that is not this topology's must not lead outside the tensors
    int64_t lo = off[i], hi = off[i + 1];
    lo = lo < 0 ? 0 : (lo > n_adj ? n_adj : lo);
    hi = hi < lo ? lo : (hi > n_adj ? n_adj : hi);
    float x = 0.f, y = 0.f, z = 0.f;
    const float* g = gc + b * n_adj * 3;
    for (int64_t e = lo; e < hi; ++e) {
        const int64_t a = adj[e];
        if (a < 0 || a >= n_adj) continue;
        const int64_t k = a / nf, f = a % nf;
        const float* p = g + (3 * f + k) * 3;
        x = x + p[0];
        y = y + p[1];
        z = z + p[2];
    }
    float* o = gv + item * 3;
    o[0] = x, o[1] = y, o[2] = z;
}

}  // namespace

extern "C" int sr_explode_bwd(float* gv, const float* gc, const int32_t* adj_off, const int32_t* adj, int64_t B, int64_t nv,
                              int64_t nf, sr_stream_t stream) {
    if (B < 0 || nv < 0 || nf < 0) return SR_EINVAL;
    if (B > 65535 || nv >= (1LL << 31) || 3 * nf >= (1LL << 31) || B * nv >= (1LL << 38)) return SR_ERANGE;
    if (B == 0 || nv == 0) return SR_OK;
    if (!gv || !adj_off || (nf > 0 && (!gc || !adj)) || gv == gc) return SR_EINVAL;
    hipLaunchKernelGGL(k_explode_bwd, dim3((unsigned)sr_ceil_div(B * nv, EX_BLOCK)), dim3(EX_BLOCK), 0, sr_stream(stream), gv,
                       gc, adj_off, adj, B, nv, nf);
    return sr_launch_status();
}
