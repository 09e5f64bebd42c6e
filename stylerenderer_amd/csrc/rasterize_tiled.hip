// LDS-tiled forward of the rasterizer: the kernels and their launch (rasterize_tiled.h has the algorithm).
#include "rasterize_tiled.h"

#include <stdlib.h>

namespace {

// (also resets the gradient state of the call when there is one: the big-triangle counter, the leader table
// `first`, which k_tile_raster fills while it resolves its tiles, and the state word behind it: 1 = table built by the
// forward pass)
__global__ __launch_bounds__(256) void k_tile_zero(unsigned* __restrict__ p, long long n, int* __restrict__ big,
                                                   int* __restrict__ first, long long n_first) {
    if (big && blockIdx.x == 0 && threadIdx.x == 0) {
        *big = 0;
        if (first) first[n_first] = 1;
    }
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) p[i] = 0u;
    if (first)
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_first; i += stride) first[i] = 0x7FFFFFFF;
}

// Wave-level aggregation of counter increments, split so that the atomics of several groups are in flight together:
// `wave_group` only votes (no memory operation): the lanes of `active` that share `idx` form a group; returns the mask
// of the caller's group.  The lowest lane of a group issues ONE atomicAdd(count of the group) — every group of the wave
// in the same instruction — and the others fetch the base from it (`wave_slot`).
__device__ __forceinline__ unsigned long long wave_group(unsigned idx, bool active) {
    unsigned long long mine = 0;
    unsigned long long todo = __ballot(active);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const unsigned key = (unsigned)__shfl((int)idx, lead, SR_WAVE);
        const unsigned long long same = __ballot(active && idx == key) & todo;
        if ((same >> lane) & 1ull) mine = same;
        todo &= ~same;
    }
    return mine;
}
__device__ __forceinline__ unsigned wave_slot(unsigned long long group, unsigned leader_base) {
    const int lane = threadIdx.x & 63;
    const int lead = group ? __ffsll((long long)group) - 1 : lane;
    const unsigned base = (unsigned)__shfl((int)leader_base, lead, SR_WAVE);
    return base + (unsigned)__popcll(group & ((1ull << lane) - 1ull));
}

// grid (ceil(nf / 256), b)
template <bool PERSP>
__global__ __launch_bounds__(256) void k_tile_bin(unsigned nv, unsigned nf, int res, bool repeat_v, bool repeat_f,
                                                  const float* __restrict__ v, const long long* __restrict__ f,
                                                  unsigned* __restrict__ tile_cnt, unsigned* __restrict__ tile_list,
                                                  unsigned* __restrict__ wide_cnt, unsigned* __restrict__ wide_list,
                                                  int* __restrict__ big, int ntx, float eps) {
    const unsigned ti = blockIdx.x * 256 + threadIdx.x;
    const unsigned s = blockIdx.y;
    Tri<float> t;
    bool ok = false;
    if (ti < nf) {
        const float* vs = repeat_v ? v : v + (size_t)s * nv * 3;
        const long long* fs = repeat_f ? f : f + (size_t)s * nf * 3;
        unsigned i0, i1, i2;
        ok = load_tri32(t, vs, fs, ti, nv, i0, i1, i2) && tri_bounds_fast<PERSP>(t, res, eps);
    }
    bool wide = ok && ((long long)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > BIG_BOX);
    if (wide && big) big[1 + atomicAdd(big, 1)] = (int)(s * nf + ti);   // (gradient pass: one row each, any order)
    const int ntile = ntx * ntx;
    const bool small_ok = ok && !wide;
    const int tx0 = small_ok ? t.x0 / TILE : 0, tx1 = small_ok ? t.x1 / TILE : 0;
    const int ty0 = small_ok ? t.y0 / TILE : 0, ty1 = small_ok ? t.y1 / TILE : 0;
    const int lane = threadIdx.x & 63;
    // a small box (<= 64 pixels) touches <= 4 tiles: 2 x 2, or up to 3 in a row.  The four common steps vote first and
    // then have their counter atomics in flight together (a returning atomic is a ~microsecond round trip)
    const bool h00 = small_ok, h01 = small_ok && tx0 + 1 <= tx1, h10 = small_ok && ty0 + 1 <= ty1, h11 = h01 && h10;
    const unsigned base_tile = s * ntile + ty0 * ntx + tx0;
    const unsigned t00 = base_tile, t01 = base_tile + 1, t10 = base_tile + ntx, t11 = base_tile + ntx + 1;
    const unsigned long long g00 = wave_group(t00, h00), g01 = wave_group(t01, h01), g10 = wave_group(t10, h10),
                             g11 = wave_group(t11, h11);
    unsigned b00 = 0, b01 = 0, b10 = 0, b11 = 0;
    if (g00 && lane == __ffsll((long long)g00) - 1) b00 = atomicAdd(&tile_cnt[t00], (unsigned)__popcll(g00));
    if (g01 && lane == __ffsll((long long)g01) - 1) b01 = atomicAdd(&tile_cnt[t01], (unsigned)__popcll(g01));
    if (g10 && lane == __ffsll((long long)g10) - 1) b10 = atomicAdd(&tile_cnt[t10], (unsigned)__popcll(g10));
    if (g11 && lane == __ffsll((long long)g11) - 1) b11 = atomicAdd(&tile_cnt[t11], (unsigned)__popcll(g11));
    const unsigned s00 = wave_slot(g00, b00), s01 = wave_slot(g01, b01), s10 = wave_slot(g10, b10),
                   s11 = wave_slot(g11, b11);
#define SR_TILE_PUT(H, T, S)                                                        \
    if (H) {                                                                        \
        if ((S) < (unsigned)TILE_CAP) tile_list[(size_t)(T) * TILE_CAP + (S)] = ti; \
        else wide = true; /* this tile is full: every tile of the sample scans it */ \
    }
    SR_TILE_PUT(h00, t00, s00)
    SR_TILE_PUT(h01, t01, s01)
    SR_TILE_PUT(h10, t10, s10)
    SR_TILE_PUT(h11, t11, s11)
    // third tile of a 1-pixel-high / -wide strip (rare)
    const bool h02 = small_ok && tx0 + 2 <= tx1, h20 = small_ok && ty0 + 2 <= ty1;
    if (__ballot(h02 || h20)) {
        const unsigned t02 = base_tile + 2, t20 = base_tile + 2 * ntx;
        const unsigned long long g02 = wave_group(t02, h02), g20 = wave_group(t20, h20);
        unsigned b02 = 0, b20 = 0;
        if (g02 && lane == __ffsll((long long)g02) - 1) b02 = atomicAdd(&tile_cnt[t02], (unsigned)__popcll(g02));
        if (g20 && lane == __ffsll((long long)g20) - 1) b20 = atomicAdd(&tile_cnt[t20], (unsigned)__popcll(g20));
        const unsigned s02 = wave_slot(g02, b02), s20 = wave_slot(g20, b20);
        SR_TILE_PUT(h02, t02, s02)
        SR_TILE_PUT(h20, t20, s20)
    }
#undef SR_TILE_PUT
    if (__ballot(wide)) {
        const unsigned long long gw = wave_group(s, wide);
        unsigned bw = 0;
        if (gw && lane == __ffsll((long long)gw) - 1) bw = atomicAdd(&wide_cnt[s], (unsigned)__popcll(gw));
        const unsigned slot = wave_slot(gw, bw);
        if (wide) wide_list[(size_t)s * nf + slot] = ti;
    }
}

// The same binning with the counters of a workgroup aggregated in LDS (images of up to BIN_LDS_TILES tiles): every hit is
// one returning LDS atomic (its slot inside the workgroup's share of the tile), then ONE global atomic per tile the
// workgroup touched reserves the share, then the entries are stored.  No wave votes; 256 consecutive triangles of a mesh
// touch a handful of tiles, so the global atomics drop by the number of waves and the list stores of a tile are contiguous.
template <bool PERSP>
__global__ __launch_bounds__(256) void k_tile_bin_lds(unsigned nv, unsigned nf, int res, bool repeat_v, bool repeat_f,
                                                      const float* __restrict__ v, const long long* __restrict__ f,
                                                      unsigned* __restrict__ tile_cnt, unsigned* __restrict__ tile_list,
                                                      unsigned* __restrict__ wide_cnt, unsigned* __restrict__ wide_list,
                                                      int* __restrict__ big, int ntx, float eps) {
    __shared__ unsigned s_cnt[BIN_LDS_TILES + 1], s_base[BIN_LDS_TILES + 1];       // [ntile] = the sample's wide list
    const int ntile = ntx * ntx;
    for (int i = threadIdx.x; i <= ntile; i += 256) s_cnt[i] = 0u;
    const unsigned ti = blockIdx.x * 256 + threadIdx.x;
    const unsigned s = blockIdx.y;
    Tri<float> t;
    bool ok = false;
    if (ti < nf) {
        const float* vs = repeat_v ? v : v + (size_t)s * nv * 3;
        const long long* fs = repeat_f ? f : f + (size_t)s * nf * 3;
        unsigned i0, i1, i2;
        ok = load_tri32(t, vs, fs, ti, nv, i0, i1, i2) && tri_bounds_fast<PERSP>(t, res, eps);
    }
    const bool wide0 = ok && ((long long)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > BIG_BOX);
    if (wide0 && big) big[1 + atomicAdd(big, 1)] = (int)(s * nf + ti);   // (gradient pass: one row each, any order)
    const bool small_ok = ok && !wide0;
    // a small box (<= 64 pixels) touches <= 4 tiles as 2 x 2, or up to 3 in a row / column
    const int tx0 = small_ok ? t.x0 / TILE : 0, tx1 = small_ok ? t.x1 / TILE : -1;
    const int ty0 = small_ok ? t.y0 / TILE : 0, ty1 = small_ok ? t.y1 / TILE : -1;
    __syncthreads();
    int tl[6];
    unsigned slot[6];
    int n_hit = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        // (0,0) (1,0) (0,1) (1,1) (2,0) (0,2): the last two only for one-pixel-high / -wide strips
        const int dx = k == 1 || k == 3 ? 1 : (k == 4 ? 2 : 0), dy = k == 2 || k == 3 ? 1 : (k == 5 ? 2 : 0);
        const bool hit = tx0 + dx <= tx1 && ty0 + dy <= ty1;      // (3 x 2 tiles would need a box of >= 68 pixels)
        tl[k] = hit ? (ty0 + dy) * ntx + tx0 + dx : -1;
        slot[k] = hit ? atomicAdd(&s_cnt[tl[k]], 1u) : 0u;
        n_hit += hit;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ntile; i += 256) {
        const unsigned c = s_cnt[i];
        if (c) s_base[i] = atomicAdd(&tile_cnt[s * ntile + i], c);
    }
    __syncthreads();
    bool wide = wide0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (tl[k] < 0) continue;
        const unsigned pos = s_base[tl[k]] + slot[k];
        if (pos < (unsigned)TILE_CAP) tile_list[(size_t)(s * ntile + tl[k]) * TILE_CAP + pos] = ti;
        else wide = true;                   // this tile is full: every tile of the sample scans the triangle
    }
    const unsigned wslot = wide ? atomicAdd(&s_cnt[ntile], 1u) : 0u;
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt[ntile]) s_base[ntile] = atomicAdd(&wide_cnt[s], s_cnt[ntile]);
    __syncthreads();
    if (wide) wide_list[(size_t)s * nf + s_base[ntile] + wslot] = ti;
}

// Exclusive prefix sum of one int per lane over the 256 lanes; returns the lane's offset, total in `total`.
__device__ __forceinline__ int block_scan_256(int x, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(incl, off, SR_WAVE);
        if (lane >= off) incl += y;
    }
    __syncthreads();                       // (s_wave may still be read from the previous round)
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    const int w0 = s_wave[0], w1 = s_wave[1], w2 = s_wave[2], w3 = s_wave[3];
    total = w0 + w1 + w2 + w3;
    const int before = (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0);
    return before + incl - x;
}

template <bool PERSP>
__global__ __launch_bounds__(256) void k_tile_raster(unsigned b, unsigned nv, unsigned nf, int res, bool repeat_v,
                                                     bool repeat_f, const float* __restrict__ v,
                                                     const long long* __restrict__ f,
                                                     const unsigned* __restrict__ tile_cnt,
                                                     const unsigned* __restrict__ tile_list,
                                                     const unsigned* __restrict__ wide_cnt,
                                                     const unsigned* __restrict__ wide_list, int ntx,
                                                     long long* __restrict__ index, float* __restrict__ coeff,
                                                     float* __restrict__ zbuf, const float* __restrict__ tex,
                                                     int tex_c, float* __restrict__ attr, int* __restrict__ win,
                                                     int* __restrict__ first, float eps, bool chw) {
    __shared__ unsigned long long s_key[TILE * TILE];
    __shared__ float s_rec[REC_F][256];
    __shared__ int s_box[4][256];          // clipped box x0, y0, width; triangle id
    __shared__ int s_pre[257];
    __shared__ int s_wave[4];
    const unsigned ntile = (unsigned)(ntx * ntx);
    // all tiles of a sample on one XCD (blockIdx round-robins over the 8 XCDs): its vertices stay in that L2
    const unsigned nblk = b * ntile;
    unsigned unit = blockIdx.x;
    {
        const unsigned per = nblk / SR_NUM_XCD;
        if (per * SR_NUM_XCD == nblk) unit = (blockIdx.x % SR_NUM_XCD) * per + blockIdx.x / SR_NUM_XCD;
    }
    const unsigned s = unit / ntile;
    const int tile = (int)(unit - s * ntile);
    const int ox = (tile % ntx) * TILE, oy = (tile / ntx) * TILE;
    const float* vs = repeat_v ? v : v + (size_t)s * nv * 3;
    const long long* fs = repeat_f ? f : f + (size_t)s * nf * 3;
    for (int i = threadIdx.x; i < TILE * TILE; i += 256) s_key[i] = key_init_f32();
    __syncthreads();
    unsigned n_own = tile_cnt[s * ntile + tile];
    if (n_own > (unsigned)TILE_CAP) n_own = TILE_CAP;
    const unsigned n_wide = wide_cnt[s];
    const unsigned* own = tile_list + (size_t)(s * ntile + tile) * TILE_CAP;
    const unsigned* wl = wide_list + (size_t)s * nf;
    const unsigned n_all = n_own + n_wide;
    for (unsigned c0 = 0; c0 < n_all; c0 += 256) {
        const unsigned e = c0 + threadIdx.x;
        int npx = 0;
        if (e < n_all) {
            const unsigned ti = e < n_own ? own[e] : wl[e - n_own];
            Tri<float> t;
            unsigned i0, i1, i2;
            load_tri32(t, vs, fs, ti, nv, i0, i1, i2);
            tri_setup_accepted<PERSP>(t, res, eps, true);          // accepted in k_tile_bin: same inputs, same bits
            const int x0 = t.x0 > ox ? t.x0 : ox, x1 = t.x1 < ox + TILE - 1 ? t.x1 : ox + TILE - 1;
            const int y0 = t.y0 > oy ? t.y0 : oy, y1 = t.y1 < oy + TILE - 1 ? t.y1 : oy + TILE - 1;
            if (x1 >= x0 && y1 >= y0) npx = (x1 - x0 + 1) * (y1 - y0 + 1);
            const int l = threadIdx.x;
            s_rec[0][l] = t.p2; s_rec[1][l] = t.p5; s_rec[2][l] = t.p8;
            s_rec[3][l] = t.e0; s_rec[4][l] = t.e1; s_rec[5][l] = t.e2; s_rec[6][l] = t.e3; s_rec[7][l] = t.e4;
            s_rec[8][l] = t.e5; s_rec[9][l] = t.e6; s_rec[10][l] = t.e7; s_rec[11][l] = t.e8; s_rec[12][l] = t.area;
            s_box[0][l] = x0; s_box[1][l] = y0; s_box[3][l] = (int)ti;
            // box width and ceil(2^16 / width): item -> row is a multiply + shift (exact: item < 1024, width <= 32)
            // (a wide-list triangle whose clipped box misses this tile has npx = 0 and possibly x1 = x0 - 1: nothing reads
            // its entry, and the division is not evaluated)
            s_box[2][l] = npx > 0 ? (x1 - x0 + 1) | ((65536 + (x1 - x0)) / (x1 - x0 + 1)) << 8 : 0;
        }
        int total;
        const int before = block_scan_256(npx, s_wave, total);
        s_pre[threadIdx.x] = before;
        if (threadIdx.x == 255) s_pre[256] = total;
        __syncthreads();
        for (int item = threadIdx.x; item < total; item += 256) {
            int lo = 0, hi = 256;                       // largest j with s_pre[j] <= item
#pragma unroll
            for (int step = 0; step < 8; ++step) {
                const int mid = (lo + hi) >> 1;
                if (s_pre[mid] <= item) lo = mid; else hi = mid;
            }
            const int j = lo, local = item - s_pre[j];
            const int bwr = s_box[2][j], bw = bwr & 0xFF;
            const int yy = (int)(((unsigned)local * (unsigned)(bwr >> 8)) >> 16), xx = local - yy * bw;
            const int x = s_box[0][j] + xx, y = s_box[1][j] + yy;
            Tri<float> t;
            t.p2 = s_rec[0][j]; t.p5 = s_rec[1][j]; t.p8 = s_rec[2][j];
            t.e0 = s_rec[3][j]; t.e1 = s_rec[4][j]; t.e2 = s_rec[5][j]; t.e3 = s_rec[6][j]; t.e4 = s_rec[7][j];
            t.e5 = s_rec[8][j]; t.e6 = s_rec[9][j]; t.e7 = s_rec[10][j]; t.e8 = s_rec[11][j]; t.area = s_rec[12][j];
            t.p0 = t.p1 = t.p3 = t.p4 = t.p6 = t.p7 = 0.0f;
            if (!(t.area > eps)) {
                // zero-area triangle (segment / point rules of pixel_weights read the screen-space vertices): rare,
                // so the record does not carry them — gathered again, same projection, same bits
                unsigned i0, i1, i2;
                Tri<float> q;
                load_tri32(q, vs, fs, (unsigned)s_box[3][j], nv, i0, i1, i2);
                screen3<PERSP>(q, (float)res, eps);
                t.p0 = q.p0; t.p1 = q.p1; t.p3 = q.p3; t.p4 = q.p4; t.p6 = q.p6; t.p7 = q.p7;
            }
            float c0, c1, c2, z;
            if (shade<float>(t, x, y, PERSP, eps, c0, c1, c2, z) && z == z) {      // NaN never passes `zB < z`
                const unsigned long long key =
                    ((unsigned long long)ord32(z) << 32) | (unsigned long long)(0xFFFFFFFEu - (unsigned)s_box[3][j]);
                unsigned long long* slot = &s_key[(y - oy) * TILE + (x - ox)];
                if (key > *slot) atomicMax(slot, key);
            }
        }
        __syncthreads();                                // records / prefix are rewritten by the next chunk
    }
    __syncthreads();
    // ---- resolve the tile from LDS: every pixel written once ----
    const size_t hw = (size_t)res * res;
    const long long shift = repeat_v ? 0 : (long long)nv * s;
    for (int p = threadIdx.x; p < TILE * TILE; p += 256) {
        const int lx = p & (TILE - 1), ly = p / TILE;
        const int x = ox + lx, y = oy + ly;
        if (x >= res || y >= res) continue;
        const unsigned long long key = s_key[p];
        int ti = -1;
        if (key != key_init_f32()) ti = (int)(0xFFFFFFFEu - (unsigned)(key & 0xFFFFFFFFull));
        unsigned i0 = 0, i1 = 0, i2 = 0;
        float c0 = 0, c1 = 0, c2 = 0, z = Lim<float>::lowest();
        long long shf = 0;
        if (ti >= 0) {
            Tri<float> t;
            load_tri32(t, vs, fs, (unsigned)ti, nv, i0, i1, i2);
            tri_setup_accepted<PERSP>(t, res, eps, false);
            shade<float>(t, x, y, PERSP, eps, c0, c1, c2, z);
            shf = shift;
        }
        const size_t g = (size_t)s * hw + (size_t)y * res + x;
        if (index) {
            index[3 * g] = (long long)i0 + shf;
            index[3 * g + 1] = (long long)i1 + shf;
            index[3 * g + 2] = (long long)i2 + shf;
        }
        if (coeff) {
            coeff[3 * g] = c0;
            coeff[3 * g + 1] = c1;
            coeff[3 * g + 2] = c2;
        }
        if (zbuf) zbuf[g] = z;
        if (win) win[g] = ti;
        if (first && ti >= 0) {
            // leader table of the gradient pass (k_first_pix's job, done here where the tile's winners sit in LDS):
            // first[sample, triangle] = smallest row-major pixel the triangle won.  A pixel whose left or upper
            // neighbour INSIDE the tile has the same winner cannot be the minimum and skips the atomic; tile-border
            // pixels always try (integer minimum: idempotent and order independent).
            const unsigned mine = (unsigned)(key & 0xFFFFFFFFull);
            const bool left = lx > 0 && (unsigned)(s_key[p - 1] & 0xFFFFFFFFull) == mine &&
                              s_key[p - 1] != key_init_f32();
            const bool up = ly > 0 && (unsigned)(s_key[p - TILE] & 0xFFFFFFFFull) == mine &&
                            s_key[p - TILE] != key_init_f32();
            if (!left && !up) atomicMin(&first[(size_t)s * nf + ti], y * res + x);
        }
        if (attr) {
            const size_t r0 = (size_t)((long long)i0 + shf) * tex_c, r1 = (size_t)((long long)i1 + shf) * tex_c,
                         r2 = (size_t)((long long)i2 + shf) * tex_c;
            for (int ch = 0; ch < tex_c; ++ch) {
                const float a0 = tex[r0 + ch] * c0;
                const float a1 = tex[r1 + ch] * c1;
                const float a2 = tex[r2 + ch] * c2;
                const float s01 = a0 + a1;
                attr[chw ? ((size_t)s * tex_c + ch) * hw + (size_t)y * res + x : g * tex_c + ch] = s01 + a2;
            }
        }
    }
}

// SR_RASTER_TILED: 0 = never, set otherwise = whenever possible, unset = by size
int tiled_mode() {
    const int c = sr_env_char("SR_RASTER_TILED");             // read per call: tests flip it at run time
    return c < 0 ? 2 : (c == '0' ? 0 : 1);
}
// SR_RASTER_BIN_LDS=0: the wave-vote binning k_tile_bin at every size (A/B, tests)
bool bin_lds_enabled() { return !sr_env_off("SR_RASTER_BIN_LDS"); }

}  // namespace

bool raster_tiled_ok(long long b, long long nf, long long h, long long w) {
    const int mode = tiled_mode();
    const long long ntx = sr_ceil_div(h, TILE), ntile = ntx * ntx;
    const bool possible = mode != 0 && h == w && nf > 0 && h < 0x40000000LL && b <= 65535 && b * ntile < 0x7FFFFFFFLL &&
                          b * nf < 0x7FFFFFFFLL;
    if (!possible) return false;
    return mode == 1 || (b * ntile >= 4096 && nf <= 1024 * ntile);
}

template <bool PERSP>
static void tiled_launch(const RasterForward<float>& c, const TileScratch& s, int* first, bool bin_lds, hipStream_t st) {
    const dim3 bin_grid((unsigned)sr_ceil_div(c.nf, 256), (unsigned)c.b);
    if (s.ntile <= BIN_LDS_TILES && bin_lds)
        hipLaunchKernelGGL((k_tile_bin_lds<PERSP>), bin_grid, dim3(256), 0, st, (unsigned)c.nv, (unsigned)c.nf, (int)c.h,
                           c.repeat_v, c.repeat_f, c.v, c.tri, s.tile_cnt, s.tile_list, s.wide_cnt, s.wide_list, c.big, s.ntx,
                           c.eps);
    else
        hipLaunchKernelGGL((k_tile_bin<PERSP>), bin_grid, dim3(256), 0, st, (unsigned)c.nv, (unsigned)c.nf, (int)c.h,
                           c.repeat_v, c.repeat_f, c.v, c.tri, s.tile_cnt, s.tile_list, s.wide_cnt, s.wide_list, c.big, s.ntx,
                           c.eps);
    hipLaunchKernelGGL((k_tile_raster<PERSP>), dim3((unsigned)(c.b * s.ntile)), dim3(256), 0, st, (unsigned)c.b,
                       (unsigned)c.nv, (unsigned)c.nf, (int)c.h, c.repeat_v, c.repeat_f, c.v, c.tri, s.tile_cnt, s.tile_list,
                       s.wide_cnt, s.wide_list, s.ntx, c.index, c.coeff, c.zbuf, c.tex, (int)c.tex_c, c.attr, c.win, first,
                       c.eps, c.chw);
}

int raster_tiled_launch(const RasterForward<float>& c, void* work, hipStream_t st) {
    const TileScratch s = tile_scratch(work, c.b, c.nf, c.h);
    int* first = (c.big && c.win) ? grad_state(c.big, c.b, c.nf).leaders : nullptr;
    hipLaunchKernelGGL(k_tile_zero, dim3(sr_stream_grid(first ? c.b * c.nf : s.counters, 256)), dim3(256), 0, st, s.tile_cnt,
                       s.counters, c.big, first, c.b * c.nf);
    const bool bin_lds = bin_lds_enabled();
    if (c.perspective) tiled_launch<true>(c, s, first, bin_lds, st);
    else tiled_launch<false>(c, s, first, bin_lds, st);
    return sr_launch_status();
}
