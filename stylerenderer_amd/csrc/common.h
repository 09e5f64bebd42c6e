// Shared helpers for the gfx950 kernels of libstylerenderer_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "../../include/stylerenderer_amd.h"

#define SR_WAVE 64          // CDNA wavefront width
#define SR_NUM_CU 256       // MI355X
#define SR_NUM_XCD 8

static inline hipStream_t sr_stream(sr_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Launch-error check: no host synchronisation, just the enqueue status.
static inline int sr_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SR_OK : static_cast<int>(e);
}

static inline int64_t sr_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Memory-bound grid sizing: enough workgroups to fill 256 CUs several times over, then
// grid-stride (guide §6 G11).
static inline int sr_stream_grid(int64_t work_items, int per_block) {
    int64_t g = sr_ceil_div(work_items, per_block);
    const int64_t cap = (int64_t)SR_NUM_CU * 16;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return static_cast<int>(g);
}

// Run-time switches live in the environment and are read per call (tests flip them between calls).
// First character of a switch's value: -1 when it is not set, 0 when it is set to the empty string.
static inline int sr_env_char(const char* name) {
    const char* e = std::getenv(name);
    return e ? (unsigned char)e[0] : -1;
}
// A switch is off when its value starts with '0'.
static inline bool sr_env_off(const char* name) { return sr_env_char(name) == '0'; }

static inline bool sr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// V = 4: one 16-byte load of four floats (p 16-byte aligned); V = 1: one float
template <int V>
__device__ __forceinline__ void sr_load_v(float* o, const float* p) {
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    } else {
        o[0] = p[0];
    }
}

// wave64 sum via DPP-friendly shuffles
__device__ __forceinline__ float sr_wave_sum(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, SR_WAVE);
    return x;
}

// Last word of a raw buffer resource (gfx9 DATA_FORMAT = 32-bit): out-of-range offsets are checked against the size in bytes
constexpr int SR_BUF_RSRC_WORD3 = 0x00020000;

#if __HIP_DEVICE_COMPILE__
// Buffer resource over [base, base + bytes) for raw buffer loads / LDS-DMA.  Every input goes through readfirstlane
// so that the descriptor provably lives in SGPRs: a descriptor the compiler believes divergent turns each buffer
// operation into a waterfall loop.  The builtins exist in the device pass only, hence the guard (kernels that use
// them keep their bodies under the same guard; the host pass needs just the launch stub).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const float* base, int bytes) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0,
                                             __builtin_amdgcn_readfirstlane(bytes), SR_BUF_RSRC_WORD3);
}
#endif
