// Measuring instances on the device: per (image, label) area, box, raw moments, crack perimeter, first pixel and colour
// sums of a uint8 label map, the derived measurements, and filtering / ordering / renumbering instances by them.
//   isa_label_props   : acc[i][v][0..15] (int64) from one pass over the map, set to the empty values by the entry itself;
//   isa_instance_props: out[i][v][0..23] (double) from acc, one workgroup per image, thread v = label v;
//   isa_props_select  : table[i][0..255] (old label -> new label), count, dropped, from acc; same launch shape;
//   isa_relabel_u8    : out = table[labels].
// The accumulation has the shape of pair_hist_kernel (score.hip): a map of L pixels is cut into S <= ISA_ROW_CHUNKS
// chunks, one 256-thread workgroup each, read 4 or 16 pixels per lane and trip.  A lane merges its pixels into horizontal
// runs of one label (cut at a row end: with w % 16 != 0 a lane's pixels straddle rows) and adds a run to the label's LDS
// row with closed forms (length, sum and sum of squares of an integer interval): about ten LDS atomics a run, none for
// background, and the minima / maxima only when the run would move them.  A lane whose pixels of a trip are all
// background pays nothing but their load: no neighbour rows, no image bytes, no atomic; any other lane issues the loads of
// the rows above and below together, and the next trip's pixels are on their way while this trip's are worked on.  The
// workgroup then adds its non-empty rows to acc
// with 64-bit integer atomics - add, min, max of integers: the result is the same whatever order workgroups run in.
#include "common.hpp"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_MIN_CHUNK = 4096;
constexpr int PR_ACC = ISA_PROPS_ACC;
constexpr int PR_OUT = ISA_PROPS_OUT;
typedef long long i64;

enum { S_AREA = 0, S_MINX, S_MAXX, S_MINY, S_MAXY, S_SX, S_SY, S_SXX, S_SYY, S_SXY, S_PERIM, S_FIRST, S_CH0 };

struct PrGeom { int L, S, chunk, h, w; };          // chunk: pixels per workgroup, a multiple of the trip

// W: 32-bit words of the map per lane and trip (1: 4 pixels, 4: 16 pixels in one 16-byte load)
bool pr_geom(int h, int w, int W, PrGeom* g) {
    const long L = (long)h * w, trip = (long)PR_THREADS * 4 * W;
    if (h <= 0 || w <= 0 || h > ISA_PROPS_MAX_SIDE || w > ISA_PROPS_MAX_SIDE || L % 4) return false;
    long S = (L + PR_MIN_CHUNK - 1) / PR_MIN_CHUNK;
    if (S > ISA_ROW_CHUNKS) S = ISA_ROW_CHUNKS;
    long chunk = (L + S - 1) / S;
    chunk = (chunk + trip - 1) / trip * trip;
    S = (L + chunk - 1) / chunk;
    *g = PrGeom{(int)L, (int)S, (int)chunk, h, w};
    return true;
}

__device__ __forceinline__ i64 empty_slot(int k, int h, int w) {
    return k == S_MINX ? w : k == S_MINY ? h : (k == S_MAXX || k == S_MAXY) ? -1 : k == S_FIRST ? (i64)h * w : 0;
}

__device__ __forceinline__ void lds_add(i64* p, i64 v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// a stale read can only be too large (too small for the maximum): then the atomic is issued without need, never skipped
__device__ __forceinline__ void lds_min(i64* p, i64 v) {
    if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
        __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_max(i64* p, i64 v) {
    if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
        __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// a horizontal run of `len` pixels of label v that starts at (x0, y); per: its crack edges, ch: its channel sums
struct Run { int v, x0, y, len, per; unsigned ch[4]; };

// sum of k^2 over 0 <= k <= n (n >= -1, n < 2^15: below 2^46)
__device__ __forceinline__ i64 sq_sum(i64 n) { return n * (n + 1) * (2 * n + 1) / 6; }

template <int C>
__device__ __forceinline__ void flush(Run& r, i64* tab, int w) {
    if (!r.len) return;
    i64* row = tab + r.v * PR_ACC;
    const i64 len = r.len, x0 = r.x0, x1 = x0 + len - 1, y = r.y;
    const i64 sx = len * (x0 + x1) / 2;                                  // len * (x0 + x1) is even for every interval
    lds_add(row + S_AREA, len);
    lds_min(row + S_MINX, x0);
    lds_max(row + S_MAXX, x1);
    lds_min(row + S_MINY, y);
    lds_max(row + S_MAXY, y);
    lds_add(row + S_SX, sx);
    lds_add(row + S_SY, y * len);
    lds_add(row + S_SXX, sq_sum(x1) - sq_sum(x0 - 1));
    lds_add(row + S_SYY, y * y * len);
    lds_add(row + S_SXY, y * sx);
    if (r.per) lds_add(row + S_PERIM, r.per);
    lds_min(row + S_FIRST, y * w + x0);
#pragma unroll
    for (int k = 0; k < C; ++k) if (r.ch[k]) lds_add(row + S_CH0 + k, r.ch[k]);
    r.len = 0;
}

// the label words of one lane and trip, the pixels [p, p + 4 W) below p1; returns the number of words that exist (L % 4 == 0:
// a word is whole or absent), the others are 0
template <int W>
__device__ __forceinline__ int load_words(const uint8_t* rl, int p, int p1, uint32_t (&wl)[W]) {
    int words = 0;
    if constexpr (W == 4) {
        if (p + 16 <= p1) {
            const uint4 v = *reinterpret_cast<const uint4*>(rl + p);
            wl[0] = v.x; wl[1] = v.y; wl[2] = v.z; wl[3] = v.w;
            words = 4;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                wl[i] = 0;
                if (p + 4 * i < p1) { wl[i] = *reinterpret_cast<const uint32_t*>(rl + p + 4 * i); words = i + 1; }
            }
        }
    } else {
        wl[0] = 0;
        if (p < p1) { wl[0] = *reinterpret_cast<const uint32_t*>(rl + p); words = 1; }
    }
    return words;
}

__global__ __launch_bounds__(PR_THREADS) void props_init_kernel(i64* acc, int32_t* oob, long slots, int n, int h, int w) {
    const long i = (long)blockIdx.x * PR_THREADS + threadIdx.x;
    if (i < slots) acc[i] = empty_slot((int)(i % PR_ACC), h, w);
    if (i < n) oob[i] = 0;
}

// C: image channels (0: no image)
template <int W, int C>
__global__ __launch_bounds__(PR_THREADS) void props_kernel(const uint8_t* labels, const uint8_t* image, PrGeom g, int nl,
                                                           i64* acc, int32_t* oob) {
    extern __shared__ i64 tab[];                                         // [nl][PR_ACC]
    const int s = blockIdx.x, img = blockIdx.y, lane = threadIdx.x & 63;
    const int h = g.h, w = g.w;
    for (int i = threadIdx.x; i < nl * PR_ACC; i += PR_THREADS) tab[i] = empty_slot(i % PR_ACC, h, w);
    __syncthreads();
    const int p0 = s * g.chunk, p1 = min(g.L, p0 + g.chunk);
    const uint8_t* rl = labels + (long)img * g.L;
    const uint8_t* ri = C ? image + (long)img * g.L * C : nullptr;
    const bool word_rows = w % 4 == 0;                                   // then the four pixels of a word share a row
    int n_oob = 0;
    constexpr int TRIP = PR_THREADS * 4 * W;
    // the words of the next trip are loaded before this trip's are worked on: one trip's load is always in flight
    uint32_t nxt[W];
    int nxt_words = load_words<W>(rl, p0 + (int)threadIdx.x * 4 * W, p1, nxt);
    for (int base = p0; base < p1; base += TRIP) {
        const int p = base + (int)threadIdx.x * 4 * W;
        uint32_t wl[W];
#pragma unroll
        for (int i = 0; i < W; ++i) wl[i] = nxt[i];
        const int words = nxt_words;                                     // valid words of this lane
        nxt_words = base + TRIP < p1 ? load_words<W>(rl, p + TRIP, p1, nxt) : 0;
        uint32_t any = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) any |= wl[i];
        if (!any) continue;                                              // background only: nothing to add
        int px[4 * W];
#pragma unroll
        for (int k = 0; k < 4 * W; ++k) px[k] = (wl[k / 4] >> (8 * (k % 4))) & 0xffu;
        const int valid = 4 * words;
        int y = p / w, x = p - y * w;
        // the rows above and below, a word at a time, every load issued before the first is used: a word outside the image
        // or the lane's valid words reads the lane's own first word instead (no branch around a load) and is never looked at
        uint32_t upw[W], dnw[W];
        if (word_rows) {
            int xi = x, yi = y;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const int qi = p + 4 * i;
                upw[i] = *reinterpret_cast<const uint32_t*>(rl + ((i < words && yi > 0) ? qi - w : p));
                dnw[i] = *reinterpret_cast<const uint32_t*>(rl + ((i < words && yi < h - 1) ? qi + w : p));
                xi += 4;
                if (xi >= w) { xi -= w; ++yi; }
            }
        }
        Run r;
        r.len = 0;
#pragma unroll
        for (int k = 0; k < 4 * W; ++k) {                                // a word that does not exist is 0: background
            const int q = p + k, v = px[k];
            if (v == 0) {
                flush<C>(r, tab, w);
            } else if (v >= nl) {
                ++n_oob;
                flush<C>(r, tab, w);
            } else {
                // a neighbour outside the image is -1: it differs from every label
                const int left = x == 0 ? -1 : k > 0 ? px[k > 0 ? k - 1 : 0] : (int)rl[q - 1];
                const int right = x == w - 1 ? -1 : k + 1 < valid ? px[k + 1 < 4 * W ? k + 1 : k] : (int)rl[q + 1];
                int up, down;
                if (word_rows) {
                    up = y > 0 ? (int)((upw[k / 4] >> (8 * (k % 4))) & 0xffu) : -1;
                    down = y < h - 1 ? (int)((dnw[k / 4] >> (8 * (k % 4))) & 0xffu) : -1;
                } else {
                    up = y > 0 ? (int)rl[q - w] : -1;
                    down = y < h - 1 ? (int)rl[q + w] : -1;
                }
                const int per = (left != v) + (right != v) + (up != v) + (down != v);
                unsigned ch[4] = {0, 0, 0, 0};
                if constexpr (C == 4) {
                    const uint32_t t = *reinterpret_cast<const uint32_t*>(ri + (long)q * 4);
                    ch[0] = t & 0xffu; ch[1] = (t >> 8) & 0xffu; ch[2] = (t >> 16) & 0xffu; ch[3] = t >> 24;
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c) ch[c] = ri[(long)q * C + c];
                }
                if (r.len && r.v == v && x != 0) {                       // the pixel before it, same row, same label
                    ++r.len;
                    r.per += per;
#pragma unroll
                    for (int c = 0; c < C; ++c) r.ch[c] += ch[c];
                } else {
                    flush<C>(r, tab, w);
                    r.v = v; r.x0 = x; r.y = y; r.len = 1; r.per = per;
#pragma unroll
                    for (int c = 0; c < 4; ++c) r.ch[c] = ch[c];
                }
            }
            if (++x == w) { x = 0; ++y; }
        }
        flush<C>(r, tab, w);                                             // the lane's next trip is not its neighbour
    }
    n_oob = wave_sum(n_oob);
    if (lane == 0 && n_oob) atomicAdd(oob + img, n_oob);
    __syncthreads();
    // thread v adds row v (label 0 is never accumulated: its row stays empty)
    const int v = threadIdx.x;
    if (v == 0 || v >= nl || tab[v * PR_ACC + S_AREA] == 0) return;
    const i64* row = tab + v * PR_ACC;
    i64* dst = acc + ((long)img * nl + v) * PR_ACC;
#pragma unroll
    for (int k = 0; k < PR_ACC; ++k) {
        const i64 t = row[k];
        if (k == S_MINX || k == S_MINY || k == S_FIRST)
            __hip_atomic_fetch_min(dst + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (k == S_MAXX || k == S_MAXY)
            __hip_atomic_fetch_max(dst + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (t)
            __hip_atomic_fetch_add(dst + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- isa_instance_props ---------------------------------------------------------------------------------------------
// a 128-bit integer as a double: two conversions and one addition, each correctly rounded
__device__ __forceinline__ double to_double(__int128 t) {
    const bool neg = t < 0;
    const unsigned __int128 u = neg ? -(unsigned __int128)t : (unsigned __int128)t;
    const double d = (double)(unsigned long long)(u >> 64) * 18446744073709551616.0 + (double)(unsigned long long)u;
    return neg ? -d : d;
}

__global__ __launch_bounds__(PR_THREADS) void derive_kernel(const i64* acc, int nl, int h, int w, int c, double* out) {
    const int img = blockIdx.x, v = threadIdx.x;
    if (v >= nl) return;
    const i64* a = acc + ((long)img * nl + v) * PR_ACC;
    double* o = out + ((long)img * nl + v) * PR_OUT;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const i64 A = a[S_AREA];
    if (v == 0 || A <= 0) {
        o[0] = 0.0;
        for (int k = 1; k < PR_OUT; ++k) o[k] = nan;
        return;
    }
    const double area = (double)A, a2 = area * area;
    const i64 x0 = a[S_MINX], x1 = a[S_MAXX] + 1, y0 = a[S_MINY], y1 = a[S_MAXY] + 1;
    const i64 sx = a[S_SX], sy = a[S_SY];
    // numerators of the central moments, exact: A * sum(x^2) passes 2^63 on large maps
    const __int128 nxx = (__int128)A * a[S_SXX] - (__int128)sx * sx;
    const __int128 nyy = (__int128)A * a[S_SYY] - (__int128)sy * sy;
    const __int128 nxy = (__int128)A * a[S_SXY] - (__int128)sx * sy;
    const double mxx = to_double(nxx) / a2, myy = to_double(nyy) / a2, mxy = to_double(nxy) / a2;
    const double half = 0.5 * (mxx + myy), d = 0.5 * (mxx - myy), rad = sqrt(d * d + mxy * mxy);
    const double l1 = half + rad, l2 = fmax(half - rad, 0.0);
    const double P = (double)a[S_PERIM], pi = 3.14159265358979323846;
    o[0] = area;
    o[1] = (double)x0; o[2] = (double)y0; o[3] = (double)x1; o[4] = (double)y1;
    o[5] = (double)sx / area; o[6] = (double)sy / area;
    o[7] = mxx; o[8] = myy; o[9] = mxy;
    o[10] = 4.0 * sqrt(l1); o[11] = 4.0 * sqrt(l2);
    o[12] = l1 == 0.0 ? 0.0 : sqrt(fmax(1.0 - l2 / l1, 0.0));
    o[13] = (mxy == 0.0 && mxx == myy) ? 0.0 : 0.5 * atan2(2.0 * mxy, mxx - myy);
    o[14] = P;
    o[15] = (x0 == 0 || y0 == 0 || x1 == w || y1 == h) ? 1.0 : 0.0;
    o[16] = area / (double)((x1 - x0) * (y1 - y0));
    o[17] = sqrt(4.0 * area / pi);
    o[18] = 4.0 * pi * area / (P * P);
    o[19] = (double)a[S_FIRST];
    for (int k = 0; k < 4; ++k) o[20 + k] = k < c ? (double)a[S_CH0 + k] / area : nan;
}

// ---- isa_props_select -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PR_THREADS) void select_kernel(const i64* acc, int nl, int h, int w, int min_area, int max_area,
                                                            int clear_border, int order, int max_objects, uint8_t* table,
                                                            int32_t* count, int32_t* dropped) {
    __shared__ i64 key[PR_THREADS];
    __shared__ int present, kept;
    const int img = blockIdx.x, v = threadIdx.x;
    constexpr i64 NONE = 0x7fffffffffffffffLL;
    if (v == 0) { present = 0; kept = 0; }
    __syncthreads();
    i64 k = NONE;
    if (v >= 1 && v < nl) {
        const i64* a = acc + ((long)img * nl + v) * PR_ACC;
        const i64 A = a[S_AREA];
        if (A > 0) {
            atomicAdd(&present, 1);
            const bool border = a[S_MINX] == 0 || a[S_MINY] == 0 || a[S_MAXX] == w - 1 || a[S_MAXY] == h - 1;
            if (A >= min_area && (max_area == 0 || A <= max_area) && !(clear_border && border)) {
                atomicAdd(&kept, 1);
                // a strict order: the old label breaks every tie
                k = order == ISA_ORDER_AREA ? ((0x7fffffffLL - A) << 8) | v : order == ISA_ORDER_RASTER ? (a[S_FIRST] << 8) | v : v;
            }
        }
    }
    key[v] = k;
    __syncthreads();
    int rank = 0;
    if (k != NONE)
        for (int u = 1; u < nl; ++u) rank += key[u] < k;
    table[(long)img * 256 + v] = (k != NONE && rank < max_objects) ? (uint8_t)(rank + 1) : (uint8_t)0;
    if (v == 0) {
        const int cnt = min(kept, max_objects);
        count[img] = cnt;
        dropped[img] = present - cnt;
    }
}

// ---- isa_relabel_u8 -------------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(PR_THREADS) void relabel_kernel(const uint8_t* labels, const uint8_t* table, long L, uint8_t* out) {
    __shared__ uint8_t tab[256];
    const int img = blockIdx.y;
    tab[threadIdx.x] = table[(long)img * 256 + threadIdx.x];
    __syncthreads();
    const uint8_t* src = labels + (long)img * L;
    uint8_t* dst = out + (long)img * L;
    const long step = (long)gridDim.x * PR_THREADS * 4 * W;
    // a lane reads its pixels before it writes them, and no other lane touches them: out == labels is fine
    for (long p = ((long)blockIdx.x * PR_THREADS + threadIdx.x) * 4 * W; p < L; p += step) {
        uint32_t wv[W];
        if constexpr (W == 4) {
            const uint4 t = *reinterpret_cast<const uint4*>(src + p);
            wv[0] = t.x; wv[1] = t.y; wv[2] = t.z; wv[3] = t.w;
        } else {
            wv[0] = *reinterpret_cast<const uint32_t*>(src + p);
        }
#pragma unroll
        for (int i = 0; i < W; ++i)
            wv[i] = (uint32_t)tab[wv[i] & 0xffu] | (uint32_t)tab[(wv[i] >> 8) & 0xffu] << 8 |
                    (uint32_t)tab[(wv[i] >> 16) & 0xffu] << 16 | (uint32_t)tab[wv[i] >> 24] << 24;
        if constexpr (W == 4) *reinterpret_cast<uint4*>(dst + p) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
        else *reinterpret_cast<uint32_t*>(dst + p) = wv[0];
    }
}

bool acc_args_ok(const void* acc, int n, int nl, int h, int w) {
    return acc && n > 0 && n <= 65535 && nl >= 1 && nl <= 256 && h > 0 && w > 0 && h <= ISA_PROPS_MAX_SIDE &&
           w <= ISA_PROPS_MAX_SIDE;
}

}  // namespace

extern "C" int isa_label_props(const uint8_t* labels, const uint8_t* image, int32_t n, int32_t h, int32_t w, int32_t c,
                               int32_t nl, int64_t* acc, int32_t* oob, void* stream) {
    if (!labels || !oob || !acc_args_ok(acc, n, nl, h, w) || (c != 0 && c != 1 && c != 3 && c != 4) || (c == 0) != !image)
        return ISA_EINVAL;
    if (!aligned(labels, 4) || !aligned(acc, 8) || !aligned(oob, 4) || (c == 4 && !aligned(image, 4))) return ISA_EALIGN;
    const bool wide = ((long)h * w) % 16 == 0 && aligned(labels, 16);
    PrGeom g;
    if (!pr_geom(h, w, wide ? 4 : 1, &g)) return ISA_EINVAL;
    hipStream_t st = as_stream(stream);
    const long slots = (long)n * nl * PR_ACC;
    hipLaunchKernelGGL(props_init_kernel, dim3(cdiv(slots, PR_THREADS)), dim3(PR_THREADS), 0, st,
                       reinterpret_cast<i64*>(acc), oob, slots, n, h, w);
    const dim3 grid(g.S, n), block(PR_THREADS);
    const size_t lds = (size_t)nl * PR_ACC * sizeof(i64);
    by_flag(wide, [&](auto wd) {
        constexpr int W = decltype(wd)::value ? 4 : 1;
#define PR_LAUNCH(C) hipLaunchKernelGGL((props_kernel<W, C>), grid, block, lds, st, labels, image, g, nl, \
                                        reinterpret_cast<i64*>(acc), oob)
        if (c == 0) PR_LAUNCH(0); else if (c == 1) PR_LAUNCH(1); else if (c == 3) PR_LAUNCH(3); else PR_LAUNCH(4);
#undef PR_LAUNCH
    });
    return launch_status();
}

extern "C" int isa_instance_props(const int64_t* acc, int32_t n, int32_t nl, int32_t h, int32_t w, int32_t c, double* out,
                                  void* stream) {
    if (!out || !acc_args_ok(acc, n, nl, h, w) || c < 0 || c > 4 || c == 2) return ISA_EINVAL;
    if (!aligned(acc, 8) || !aligned(out, 8)) return ISA_EALIGN;
    hipLaunchKernelGGL(derive_kernel, dim3(n), dim3(PR_THREADS), 0, as_stream(stream), reinterpret_cast<const i64*>(acc), nl,
                       h, w, c, out);
    return launch_status();
}

extern "C" int isa_props_select(const int64_t* acc, int32_t n, int32_t nl, int32_t h, int32_t w, int32_t min_area,
                                int32_t max_area, int32_t clear_border, int32_t order, int32_t max_objects, uint8_t* table,
                                int32_t* count, int32_t* dropped, void* stream) {
    if (!table || !count || !dropped || !acc_args_ok(acc, n, nl, h, w) || min_area < 0 || max_area < 0 ||
        (clear_border != 0 && clear_border != 1) || order < ISA_ORDER_LABEL || order > ISA_ORDER_RASTER || max_objects < 1 ||
        max_objects > 255)
        return ISA_EINVAL;
    if (!aligned(acc, 8) || !aligned(count, 4) || !aligned(dropped, 4)) return ISA_EALIGN;
    hipLaunchKernelGGL(select_kernel, dim3(n), dim3(PR_THREADS), 0, as_stream(stream), reinterpret_cast<const i64*>(acc), nl,
                       h, w, min_area, max_area, clear_border, order, max_objects, table, count, dropped);
    return launch_status();
}

extern "C" int isa_relabel_u8(const uint8_t* labels, const uint8_t* table, int32_t n, int64_t L, uint8_t* out, void* stream) {
    if (!labels || !table || !out || n <= 0 || n > 65535 || L <= 0 || L % 4 || L >= (1ll << 31)) return ISA_EINVAL;
    const uintptr_t bytes = (uintptr_t)n * (uintptr_t)L;
    // the same map or two apart, nothing between
    if (labels != out && ranges_overlap(labels, bytes, out, bytes)) return ISA_EINVAL;
    if (!aligned(labels, 4) || !aligned(out, 4)) return ISA_EALIGN;
    const bool wide = L % 16 == 0 && aligned(labels, 16) && aligned(out, 16);
    const long per_block = (long)PR_THREADS * (wide ? 16 : 4);
    const dim3 grid(grid_cap((L + per_block - 1) / per_block, 1024), n), block(PR_THREADS);
    hipStream_t st = as_stream(stream);
    if (wide) hipLaunchKernelGGL(relabel_kernel<4>, grid, block, 0, st, labels, table, (long)L, out);
    else hipLaunchKernelGGL(relabel_kernel<1>, grid, block, 0, st, labels, table, (long)L, out);
    return launch_status();
}
