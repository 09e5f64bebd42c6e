// The last kernel of the K-sliced weight-gradient paths (k_wgrad_mfma, k_wgrad_s2_dma and the two split-bf16 kernels):
// adds the partial slabs [ks][nt][UP][VP] the slices wrote, in slice order (deterministic; no float atomics), and
// writes the output layout.
#include "mfma_tile.h"
#include "conv_wgrad_reduce.h"

namespace {

// Sums the K slices in a fixed order and writes the requested layout: element (t, u, v) goes to
// out[tmap[t] * slab + u * su + v * sv].
struct ReduceParams {
    const float* partial;
    float* out;
    int ks, nt, UP, VP, CU, CV;
    int64_t slab, su, sv;
    int tmap[9];
};

__global__ __launch_bounds__(256) void k_wgrad_reduce(const ReduceParams p) {
    const int64_t total = (int64_t)p.nt * p.CU * p.CV;
    const int64_t stride_s = (int64_t)p.nt * p.UP * p.VP;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int v = (int)(i % p.CV);
        const int u = (int)((i / p.CV) % p.CU);
        const int t = (int)(i / ((int64_t)p.CV * p.CU));
        const float* src = p.partial + ((int64_t)t * p.UP + u) * p.VP + v;
        float acc = 0.0f;
#pragma unroll 8
        for (int s = 0; s < p.ks; ++s) acc += src[s * stride_s];      // loads in flight, fixed summation order
        int slab = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (t == k) slab = p.tmap[k];
        p.out[slab * p.slab + u * p.su + v * p.sv] = acc;
    }
}

// The same reduction for FEW outputs over MANY slices (the tiny-channel layers of the map heads: 12 ... 144 outputs, up to
// 512 slices): one wave per output, lane l adds slices l, l + 64, ... in order, then the wave's fixed-order sum — instead of
// one lane walking 512 slices (10 us in a single workgroup).
__global__ __launch_bounds__(256) void k_wgrad_reduce_wave(const ReduceParams p) {
    const int64_t total = (int64_t)p.nt * p.CU * p.CV;
    const int64_t stride_s = (int64_t)p.nt * p.UP * p.VP;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= total) return;
    const int v = (int)(i % p.CV);
    const int u = (int)((i / p.CV) % p.CU);
    const int t = (int)(i / ((int64_t)p.CV * p.CU));
    const float* src = p.partial + ((int64_t)t * p.UP + u) * p.VP + v;
    float acc = 0.0f;
    for (int s = lane; s < p.ks; s += 64) acc += src[s * stride_s];
    acc = sr_wave_sum(acc);
    if (lane != 0) return;
    int slab = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        if (t == k) slab = p.tmap[k];
    p.out[slab * p.slab + u * p.su + v * p.sv] = acc;
}

inline void launch_wgrad_reduce(const ReduceParams& r, int64_t total, hipStream_t st) {
    if (total <= 1024 && r.ks >= 32)
        hipLaunchKernelGGL(k_wgrad_reduce_wave, dim3((unsigned)sr_ceil_div(total, 4)), dim3(256), 0, st, r);
    else
        hipLaunchKernelGGL(k_wgrad_reduce, dim3(sr_stream_grid(total, 256)), dim3(256), 0, st, r);
}

}  // namespace

int sr_wgrad_reduce_launch(const WgradOut& out, const float* partial, int ks, int nt, int UP, int VP, int CU, int CV,
                           hipStream_t st) {
    ReduceParams r;
    r.partial = partial; r.out = out.dwt;
    r.ks = ks; r.nt = nt; r.UP = UP; r.VP = VP; r.CU = CU; r.CV = CV;
    r.slab = out.slab; r.su = out.su; r.sv = out.sv;
    for (int t = 0; t < 9; ++t) r.tmap[t] = t;
    launch_wgrad_reduce(r, (int64_t)nt * CU * CV, st);
    return sr_launch_status();
}
