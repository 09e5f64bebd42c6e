// The tap list of the texture look-up, built on the device in a fixed launch sequence (C ABI: sr_tap_plan_build,
// sr_tap_plan_scratch_ints, sr_tap_plan_passes, sr_tap_plan_digit_bits; definition: stylerenderer_amd/op/texture.py,
// tap_plan).  The list is the CSR that sr_texture_sample_bwd_tex walks: off int32 [Bt Th Tw + 2] over the texel keys
// bt Th Tw + ty Tw + tx and entries int32 [4 B H W], the taps ((b H + y) W + x) 4 + k ascending within a key, the bucket
// after the last key holding the taps of the pixels without a look-up.  It is a function of the uv map, which moves with
// every step of a fit that has the pose among its variables, so it is built per step, inside the captured iteration.
//
// A least-significant-digit radix sort of (key, entry) pairs, TP_BITS bits per pass, ceil(bits(Bt Th Tw) / TP_BITS)
// passes (the sentinel key Bt Th Tw of a pixel without taps is the largest key):
//
//   k_tap_keys      a lane per pixel: texture_footprint.h's arithmetic, the four keys in one 16-byte store.
//   per pass
//   k_tap_hist      a workgroup per tile of TP_TILE pairs: the tile's digit counts in LDS (integer LDS atomics: a count
//                   does not depend on the order of its increments), written as row `workgroup` of a [workgroups, 2^d]
//                   table.  Every element of the row is written.
//   k_tap_scan      one workgroup, a lane per digit: walks its column of the table top to bottom and replaces every count
//                   by the sum of those above it, then the 2^d column totals are scanned through LDS into base[2^d].
//                   The position of the first pair of tile g with digit q is base[q] + table[g, q]: the exclusive scan of
//                   the table in digit-major order.
//   k_tap_scatter   the same tiles.  A tile is walked in rounds of TP_BLOCK consecutive pairs.  In a round every wave
//                   finds the lanes that hold its lane's digit with TP_BITS ballots (a match mask): the rank among the
//                   equal digits of lower lanes is a population count.  The waves' counts go through LDS and are added in
//                   wave order; a running LDS counter per digit carries the rounds.  So a pair's position is its digit's
//                   base plus the number of pairs with that digit before it in input order: stable, and the same from
//                   run to run whatever the hardware retires first.  In the first pass the entry is the pair's index (no
//                   buffer is read); the last pass writes `entries`.
//   k_tap_offsets   a lane per key k in [0, Bt Th Tw + 1]: off[k] = the first position of the sorted keys that is not
//                   below k (a binary search); every element of off is written by its own lane.
//
// No workgroup waits for another: phases are ordered by kernel boundaries.  The work of every pass is a function of the
// shapes alone (a constant uv map, all taps on one key, costs what any other costs).  No float arithmetic outside the
// footprint, no global atomics, no memset, no allocation, no host read: the sequence runs under graph capture.  Nothing
// needs to start at zero; every element of the scratch that is read was written earlier in the same build.
#include "common.h"
#include "texture_footprint.h"

namespace {

constexpr int TP_BITS = 8;                      // digit width d
constexpr int TP_RADIX = 1 << TP_BITS;
constexpr int TP_BLOCK = 256;                   // == TP_RADIX: a lane per digit where digits are walked
constexpr int TP_WAVES = TP_BLOCK / SR_WAVE;
constexpr int TP_ROUNDS = 8;
constexpr int TP_TILE = TP_BLOCK * TP_ROUNDS;   // pairs per workgroup
static_assert(TP_BLOCK == TP_RADIX, "a lane per digit");

__global__ __launch_bounds__(TP_BLOCK) void k_tap_keys(int32_t* __restrict__ keys, const float* __restrict__ uv,
                                                       const uint8_t* __restrict__ cover, int64_t pixels, int64_t plane,
                                                       int64_t tplane, int per_view, int n_keys, int Th, int Tw) {
    const int64_t pix = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (pix >= pixels) return;
    const Foot f = footprint(uv[2 * pix], uv[2 * pix + 1], cover[pix] != 0, Th, Tw);
    int4 k = make_int4(n_keys, n_keys, n_keys, n_keys);
    if (f.live) {
        const int base = per_view ? (int)((pix / plane) * tplane) : 0;
        k = make_int4(base + f.o00, base + f.o01, base + f.o10, base + f.o11);
    }
    *reinterpret_cast<int4*>(keys + 4 * pix) = k;                         // (hipMalloc'd scratch, 16-byte aligned offsets)
}

__global__ __launch_bounds__(TP_BLOCK) void k_tap_hist(int32_t* __restrict__ table, const int32_t* __restrict__ keys,
                                                       int64_t n, int shift) {
    __shared__ int cnt[TP_RADIX];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t start = (int64_t)blockIdx.x * TP_TILE;
#pragma unroll
    for (int r = 0; r < TP_ROUNDS; ++r) {
        const int64_t i = start + r * TP_BLOCK + threadIdx.x;
        if (i < n) atomicAdd(&cnt[(keys[i] >> shift) & (TP_RADIX - 1)], 1);
    }
    __syncthreads();
    table[(int64_t)blockIdx.x * TP_RADIX + threadIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(TP_BLOCK) void k_tap_scan(int32_t* __restrict__ table, int32_t* __restrict__ base,
                                                       int64_t groups) {
    __shared__ int tot[TP_RADIX];
    const int q = threadIdx.x;
    int run = 0;
    for (int64_t g = 0; g < groups; ++g) {
        const int c = table[g * TP_RADIX + q];
        table[g * TP_RADIX + q] = run;
        run += c;
    }
    tot[q] = run;
    __syncthreads();
    // inclusive scan of the 2^d totals (Hillis-Steele), made exclusive by subtracting the lane's own
    for (int s = 1; s < TP_RADIX; s <<= 1) {
        const int add = q >= s ? tot[q - s] : 0;
        __syncthreads();
        tot[q] += add;
        __syncthreads();
    }
    base[q] = tot[q] - run;
}

__global__ __launch_bounds__(TP_BLOCK) void k_tap_scatter(int32_t* __restrict__ keys_out, int32_t* __restrict__ vals_out,
                                                          const int32_t* __restrict__ keys, const int32_t* vals,
                                                          const int32_t* __restrict__ table,
                                                          const int32_t* __restrict__ base, int64_t n, int shift) {
    __shared__ int at[TP_RADIX];                 // where the next pair of every digit goes
    __shared__ int wave_cnt[TP_WAVES][TP_RADIX]; // this round's count of every digit in every wave
    const int t = threadIdx.x, lane = t & (SR_WAVE - 1), wave = t / SR_WAVE;
    at[t] = base[t] + table[(int64_t)blockIdx.x * TP_RADIX + t];
    const int64_t start = (int64_t)blockIdx.x * TP_TILE;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int r = 0; r < TP_ROUNDS; ++r) {
        const int64_t i = start + r * TP_BLOCK + t;
        if (start + r * TP_BLOCK >= n) break;                             // (uniform over the workgroup)
        const bool valid = i < n;
        const int key = valid ? keys[i] : 0;
        const int val = valid ? (vals ? vals[i] : (int)i) : 0;
        const int digit = (key >> shift) & (TP_RADIX - 1);
#pragma unroll
        for (int w = 0; w < TP_WAVES; ++w) wave_cnt[w][t] = 0;
        __syncthreads();
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < TP_BITS; ++bit) {
            const bool one = (digit >> bit) & 1;
            const unsigned long long m = __ballot(one);
            same &= one ? m : ~m;
        }
        const int rank = __popcll(same & below);
        if (valid && rank == 0) wave_cnt[wave][digit] = __popcll(same);
        __syncthreads();
        if (valid) {
            int64_t pos = at[digit] + rank;
            for (int w = 0; w < wave; ++w) pos += wave_cnt[w][digit];
            if (pos >= 0 && pos < n) {                                    // (always, for a table of this build)
                keys_out[pos] = key;
                vals_out[pos] = val;
            }
        }
        __syncthreads();
        int add = 0;
#pragma unroll
        for (int w = 0; w < TP_WAVES; ++w) add += wave_cnt[w][t];
        at[t] += add;
        __syncthreads();
    }
}

__global__ __launch_bounds__(TP_BLOCK) void k_tap_offsets(int32_t* __restrict__ off, const int32_t* __restrict__ keys,
                                                          int64_t n, int64_t n_off) {
    const int64_t k = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (k >= n_off) return;
    int64_t lo = 0, hi = n;                                               // the first position whose key is >= k
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    off[k] = (int32_t)lo;
}

int plan_passes(int64_t n_keys) {
    int bits = 0;
    while ((n_keys >> bits) != 0) ++bits;                                  // the sentinel n_keys is the largest key
    return (bits + TP_BITS - 1) / TP_BITS;
}

int64_t plan_groups(int64_t n) { return sr_ceil_div(n, TP_TILE); }

int plan_check(int64_t B, int64_t Bt, int64_t H, int64_t W, int64_t Th, int64_t Tw) {
    if (B < 0 || H < 0 || W < 0 || Th < 1 || Tw < 1) return SR_EINVAL;
    if (!(Bt == B || Bt == 1)) return SR_EINVAL;
    if (B > 65535 || Bt > 65535 || H > (1 << 20) || W > (1 << 20) || Th > (1 << 20) || Tw > (1 << 20) ||
        Th * Tw >= (1LL << 31) || Bt * Th * Tw >= (1LL << 31) - 1 || 4 * B * H * W >= (1LL << 31))
        return SR_ERANGE;
    return SR_OK;
}

}  // namespace

extern "C" int sr_tap_plan_digit_bits(void) { return TP_BITS; }

extern "C" int sr_tap_plan_passes(int64_t Bt, int64_t Th, int64_t Tw) {
    if (Bt < 1 || Th < 1 || Tw < 1 || Bt > 65535 || Th > (1 << 20) || Tw > (1 << 20) || Bt * Th * Tw >= (1LL << 31) - 1)
        return -1;
    return plan_passes(Bt * Th * Tw);
}

// int32 elements: two key buffers and one entry buffer of n = 4 B H W each (n rounded up to a multiple of 4, so that
// every part starts on 16 bytes), the [workgroups, 2^d] table and base[2^d]
extern "C" int64_t sr_tap_plan_scratch_ints(int64_t B, int64_t H, int64_t W) {
    if (B < 0 || H < 0 || W < 0 || B > 65535 || H > (1 << 20) || W > (1 << 20) || 4 * B * H * W >= (1LL << 31)) return -1;
    const int64_t n = 4 * B * H * W;
    return 3 * n + plan_groups(n) * TP_RADIX + TP_RADIX;
}

extern "C" int sr_tap_plan_build(int32_t* off, int32_t* entries, int32_t* scratch, int64_t scratch_ints, const float* uv,
                                 const uint8_t* cover, int64_t B, int64_t Bt, int64_t H, int64_t W, int64_t Th, int64_t Tw,
                                 sr_stream_t stream) {
    const int rc = plan_check(B, Bt, H, W, Th, Tw);
    if (rc != SR_OK) return rc;
    if (!off) return SR_EINVAL;
    const int64_t n = 4 * B * H * W, n_keys = Bt * Th * Tw, groups = plan_groups(n);
    hipStream_t s = sr_stream(stream);
    const int32_t* sorted = nullptr;
    if (n > 0) {
        if (!entries || !scratch || !uv || !cover || !sr_aligned16(scratch)) return SR_EINVAL;
        if (scratch_ints < sr_tap_plan_scratch_ints(B, H, W)) return SR_EINVAL;
        int32_t* key_a = scratch;
        int32_t* key_b = scratch + n;
        int32_t* val_a = scratch + 2 * n;
        int32_t* table = scratch + 3 * n;
        int32_t* base = table + groups * TP_RADIX;
        const int passes = plan_passes(n_keys);
        hipLaunchKernelGGL(k_tap_keys, dim3((unsigned)sr_ceil_div(B * H * W, TP_BLOCK)), dim3(TP_BLOCK), 0, s, key_a, uv,
                           cover, B * H * W, H * W, Th * Tw, (Bt == B && B > 1) ? 1 : 0, (int)n_keys, (int)Th, (int)Tw);
        int32_t* src = key_a;
        int32_t* dst = key_b;
        for (int p = 0; p < passes; ++p) {
            // the last pass writes `entries`, the one before it val_a, and so on down
            int32_t* val_dst = ((passes - 1 - p) % 2 == 0) ? entries : val_a;
            const int32_t* val_src = p == 0 ? nullptr : (val_dst == entries ? val_a : entries);
            const int shift = p * TP_BITS;
            hipLaunchKernelGGL(k_tap_hist, dim3((unsigned)groups), dim3(TP_BLOCK), 0, s, table, src, n, shift);
            hipLaunchKernelGGL(k_tap_scan, dim3(1), dim3(TP_BLOCK), 0, s, table, base, groups);
            hipLaunchKernelGGL(k_tap_scatter, dim3((unsigned)groups), dim3(TP_BLOCK), 0, s, dst, val_dst, src, val_src, table,
                               base, n, shift);
            int32_t* tmp = src;
            src = dst;
            dst = tmp;
        }
        sorted = src;
    }
    hipLaunchKernelGGL(k_tap_offsets, dim3((unsigned)sr_ceil_div(n_keys + 2, TP_BLOCK)), dim3(TP_BLOCK), 0, s, off, sorted, n,
                       n_keys + 2);
    return sr_launch_status();
}
