// Connected components of uint8 label maps on the device, and the clean-up of instance maps built on them.
//   isa_cc_label : map uint8 [n,h,w] -> comp int32 [n,h,w] (0 = background, else 1 + the smallest row-major pixel index of
//                  the pixel's component inside its image) and n_comp int32 [n];
//   isa_cc_select: map + comp -> a renumbered uint8 label map, in mode ISA_CC_SPLIT (every component an instance, raster
//                  order) or ISA_CC_LARGEST (the largest component of every input value survives).
// Labelling is a union-find over `parent` (caller scratch, int32 [n, h*w]; a pixel index inside the image, -1 = background)
// in three launches, none of which waits for another workgroup:
//   1 tile : a workgroup labels one CC_TH x CC_TW tile in LDS and writes, for every pixel, the image index of the root of
//            its tile-local component (the tile's raster order and the image's agree inside a tile, so the local minimum is
//            the global minimum of that piece);
//   2 merge: one thread per pixel that lies on the first row or the first column of a tile unites it with its neighbours
//            across the tile edge.  Workgroups of this launch unite trees that other workgroups walk at the same time, and
//            neither a CU's L1 nor the L2 of another XCD ever sees their stores, so EVERY access to a parent word in this
//            launch, reads included, is a device-scope read-modify-write atomic (atomicMin): those are
//            performed at the memory side, in one order per word.  Skipped when the image is a single tile;
//   3 flatten: parent is final and read-only now (a launch boundary lies behind the last atomic), so plain loads follow
//            every pixel's chain to its root and write comp; the roots are counted into n_comp with integer adds.
// A union always hangs the LARGER root below the SMALLER index (atomicMin), so parent[i] <= i holds at all times, a
// component's final root is its smallest pixel, and comp does not depend on the order in which anything ran.
// Selection works on integer atomics and scans only: areas are atomic adds into area[root] (wave-aggregated, as
// pair_hist_kernel of score.hip aggregates its dominant pair), the SPLIT rank of a root is a prefix count over root pixels
// in the chunk pass + one-workgroup fold of isa_seg_claim, LARGEST winners are one 64-bit atomicMax on (area, inverted
// root) per component.
#include "common.hpp"

namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_TH = ISA_CC_TILE_H, CC_TW = ISA_CC_TILE_W, CC_TILE = CC_TH * CC_TW;
constexpr int CC_PPT = CC_TILE / CC_THREADS;         // pixels of a tile row per thread: 8 consecutive ones
constexpr int CC_MIN_CHUNK = 4096;
constexpr int CC_TRIP = CC_THREADS * 4;              // pixels per trip of a chunk pass (4 per thread)
constexpr int CC_TAB_WORDS = ISA_CC_TAB_BYTES / 4;   // per-image table of isa_cc_select, in int32 words:
constexpr int CC_TAB_KEY = 0;                        //   [0, 512)    uint64 winner key per input value (LARGEST)
constexpr int CC_TAB_ROOT = 512;                     //   [512, 768)  comp value of the surviving component per value
constexpr int CC_TAB_LAB = 768;                      //   [768, 1024) its new label
constexpr int CC_TAB_CHUNK = 1024;                   //   [1024, 1088) qualifying roots per chunk, then their exclusive scan
static_assert(CC_TW % 8 == 0 && CC_TW / CC_PPT * CC_TH == CC_THREADS && CC_PPT == 8, "a thread owns 8 pixels of a tile row");
static_assert(CC_TAB_CHUNK + ISA_ROW_CHUNKS <= CC_TAB_WORDS && ISA_CC_TAB_BYTES % 16 == 0, "table layout");

typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- union-find in LDS (tile) ----------------------------------------------------------------------------------------
// lab[i] <= i for every i at all times (it starts at i or at the start of i's run, and only atomicMin writes it).
__device__ __forceinline__ int lds_read(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(int* lab, int i) {
    // terminates: lab[i] <= i, so every step that does not stop moves to a strictly smaller index, and indices are >= 0
    int p = lds_read(lab + i);
    while (p != i) { i = p; p = lds_read(lab + i); }
    return i;
}
__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
    // terminates: a pass ends the loop, or replaces a by `old`, a value lab[a] held that is not a, hence < a; b only ever
    // moves to its root (<= b).  So a + b strictly decreases from pass to pass and is bounded by 0.  No pass waits for
    // another thread: atomicMin always completes.
    // correct: when old != a the link a -> old may just have been replaced by a -> b (old > b) or kept (old < b); either
    // way a hangs below one of them and the two still to be united are old and b.
    for (;;) {
        a = lds_find(lab, a); b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;
    }
}

// ---- union-find in global memory, between workgroups (merge) -------------------------------------------------------------
// every access is a device-scope RMW atomic; a plain or sc1 load could be served from this CU's L1 or this XCD's L2.
// The read of word i is atomicMin(par + i, i): par[i] <= i, so it changes nothing and returns the word.  (An RMW the
// compiler can prove idempotent - or 0, min INT_MAX - is folded into an atomic LOAD, which is not what is wanted here.)
__device__ __forceinline__ int g_read(int* par, int i) { return atomicMin(par + i, i); }
__device__ __forceinline__ int g_find(int* par, int i) {
    // terminates: par[i] <= i at all times (the tile launch wrote roots <= i, atomicMin only lowers), so the index followed
    // strictly decreases until a word holds its own index
    int p = g_read(par, i);
    while (p != i) { i = p; p = g_read(par, i); }
    return i;
}
__device__ __forceinline__ void g_union(int* par, int a, int b) {
    // terminates and is correct by the argument of lds_union: a + b strictly decreases, nothing waits for anyone
    for (;;) {
        a = g_find(par, a); b = g_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}

// ---- launch 1: a tile in LDS -------------------------------------------------------------------------------------------
template <bool C8>
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const uint8_t* map, int h, int w, int tiles_x, int* parent,
                                                             int* n_comp) {
    __shared__ int lab[CC_TILE];
    __shared__ uint8_t val[CC_TILE];
    if (blockIdx.x == 0 && threadIdx.x == 0) n_comp[blockIdx.y] = 0;      // the flatten launch adds to it
    const int tx0 = (int)(blockIdx.x % tiles_x) * CC_TW, ty0 = (int)(blockIdx.x / tiles_x) * CC_TH;
    const long hw = (long)h * w;
    const uint8_t* m = map + (long)blockIdx.y * hw;
    int* par = parent + (long)blockIdx.y * hw;
    const int ly = threadIdx.x / (CC_TW / CC_PPT), lx0 = (threadIdx.x % (CC_TW / CC_PPT)) * CC_PPT;
    const int gy = ty0 + ly, gx0 = tx0 + lx0, base = ly * CC_TW + lx0;
    // w % 4 == 0 and gx0 % 4 == 0: a 4-pixel word lies inside the row or outside it; outside the image counts as background
    uint32_t wd[2] = {0u, 0u};
    if (gy < h) {
        if (gx0 < w) wd[0] = *reinterpret_cast<const uint32_t*>(m + (long)gy * w + gx0);
        if (gx0 + 4 < w) wd[1] = *reinterpret_cast<const uint32_t*>(m + (long)gy * w + gx0 + 4);
    }
    int v[CC_PPT];
#pragma unroll
    for (int j = 0; j < CC_PPT; ++j) {
        v[j] = (wd[j >> 2] >> (8 * (j & 3))) & 0xffu;
        val[base + j] = (uint8_t)v[j];
    }
    // the thread's own 8 pixels: a pixel starts at the start of its run inside them
    int start = base;
#pragma unroll
    for (int j = 0; j < CC_PPT; ++j) {
        if (j == 0 || v[j] != v[j - 1]) start = base + j;
        lab[base + j] = start;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CC_PPT; ++j) {
        const int i = base + j, lx = lx0 + j, c = v[j];
        if (c == 0) continue;
        if (j == 0 && lx > 0 && val[i - 1] == c) lds_union(lab, i, i - 1);
        if (ly == 0) continue;
        const int up = i - CC_TW;
        const bool n_eq = val[up] == c;
        // north: not needed again where west and north-west already tie this column to the last one
        if (n_eq && !(j > 0 && v[j - 1] == c && val[up - 1] == c)) lds_union(lab, i, up);
        if constexpr (C8) {
            // a diagonal matters only where north differs: north and its equal-valued row neighbours are already one run
            if (!n_eq && lx > 0 && val[up - 1] == c) lds_union(lab, i, up - 1);
            if (!n_eq && lx < CC_TW - 1 && val[up + 1] == c) lds_union(lab, i, up + 1);
        }
    }
    __syncthreads();
    if (gy >= h) return;
    int out[CC_PPT];
#pragma unroll
    for (int j = 0; j < CC_PPT; ++j) {
        out[j] = -1;
        if (v[j]) {
            const int r = lds_find(lab, base + j);               // nobody writes lab any more
            out[j] = (ty0 + r / CC_TW) * w + tx0 + r % CC_TW;
        }
    }
    int* dst = par + (long)gy * w + gx0;
    if (gx0 < w) *reinterpret_cast<i32x4*>(dst) = i32x4{out[0], out[1], out[2], out[3]};
    if (gx0 + 4 < w) *reinterpret_cast<i32x4*>(dst + 4) = i32x4{out[4], out[5], out[6], out[7]};
}

// ---- launch 2: unions across tile edges ----------------------------------------------------------------------------------
// items of an image: first the pixels of the rows y = k*CC_TH (k >= 1), then those of the columns x = k*CC_TW (k >= 1).
// A row item looks north (and north-west / north-east), a column item west (and north-west / south-west): together every
// pair of neighbours that lies in two tiles, the diagonal pairs at a corner of four tiles included (some twice: harmless).
template <bool C8>
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const uint8_t* map, int h, int w, int row_items, int items,
                                                              int* parent) {
    const int item = blockIdx.x * CC_THREADS + threadIdx.x;
    if (item >= items) return;
    const long hw = (long)h * w;
    const uint8_t* m = map + (long)blockIdx.y * hw;
    int* par = parent + (long)blockIdx.y * hw;
    if (item < row_items) {
        const int y = (item / w + 1) * CC_TH, x = item % w;      // 1 <= y < h
        const int i = y * w + x, c = m[i];
        if (c == 0) return;
        const bool n_eq = m[i - w] == c;
        if (n_eq) g_union(par, i, i - w);
        if constexpr (C8) {
            // as in the tile: with an equal north pixel its row neighbours reach this pixel through it
            if (!n_eq && x > 0 && m[i - w - 1] == c) g_union(par, i, i - w - 1);
            if (!n_eq && x < w - 1 && m[i - w + 1] == c) g_union(par, i, i - w + 1);
        }
    } else {
        const int k = (item - row_items) / h, y = (item - row_items) % h, x = (k + 1) * CC_TW;      // 1 <= x < w
        const int i = y * w + x, c = m[i];
        if (c == 0) return;
        const bool w_eq = m[i - 1] == c;
        if (w_eq) g_union(par, i, i - 1);
        if constexpr (C8) {
            if (!w_eq && y > 0 && m[i - w - 1] == c) g_union(par, i, i - w - 1);
            if (!w_eq && y < h - 1 && m[i + w - 1] == c) g_union(par, i, i + w - 1);
        }
    }
}

// ---- launch 3: comp = root + 1, n_comp += roots ----------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const int* parent, long hw, int* comp, int* n_comp) {
    const long p = ((long)blockIdx.x * CC_THREADS + threadIdx.x) * 4;
    const int b = blockIdx.y;
    const int* par = parent + (long)b * hw;
    int roots = 0;
    if (p < hw) {                                                // hw % 4 == 0
        const i32x4 q = *reinterpret_cast<const i32x4*>(par + p);
        i32x4 out;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int i = q[j];
            if (i < 0) { out[j] = 0; continue; }
            if (i == (int)p + j) ++roots;
            // terminates: parent is read-only in this launch and parent[i] <= i, so the index strictly decreases to a root
            for (int nx = par[i]; nx != i; nx = par[i]) i = nx;
            out[j] = i + 1;
        }
        *reinterpret_cast<i32x4*>(comp + (long)b * hw + p) = out;
    }
    roots = wave_sum(roots);
    if ((threadIdx.x & 63) == 0 && roots) atomicAdd(n_comp + b, roots);
}

// ---- selection: chunk passes over [n, L] ------------------------------------------------------------------------------------
struct CcGeom { long L; int S; long chunk; };        // chunk: pixels per workgroup, a multiple of CC_TRIP
CcGeom cc_geom(long L) {
    long S = (L + CC_MIN_CHUNK - 1) / CC_MIN_CHUNK;
    if (S > ISA_ROW_CHUNKS) S = ISA_ROW_CHUNKS;
    long chunk = (L + S - 1) / S;
    chunk = (chunk + CC_TRIP - 1) / CC_TRIP * CC_TRIP;
    S = (L + chunk - 1) / chunk;
    return CcGeom{L, (int)S, chunk};
}

// the scratch of isa_cc_select, cleared by a launch of its own (a multiple of 16 bytes: hw % 4 == 0, ISA_CC_TAB_BYTES % 16 == 0)
__global__ __launch_bounds__(CC_THREADS) void cc_clear_kernel(i32x4* p, long vecs) {
    for (long i = (long)blockIdx.x * CC_THREADS + threadIdx.x; i < vecs; i += (long)gridDim.x * CC_THREADS)
        p[i] = i32x4{0, 0, 0, 0};
}

// area[root] += pixels.  Per trip a wave counts the component of its first lane's first pixel with ballots and adds it
// once; the other pixels are run-length merged inside the lane.  Integer adds: the order does not matter.
__global__ __launch_bounds__(CC_THREADS) void cc_area_kernel(const int* comp, CcGeom g, int* area) {
    const int s = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63;
    const long p0 = (long)s * g.chunk, p1 = min(g.L, p0 + g.chunk);
    const int* cp = comp + (long)b * g.L;
    int* ar = area + (long)b * g.L;
    int run_c = 0, run_len = 0;
    // wave-uniform trip loop: every lane runs every trip (a lane past the end holds background), the ballots see the wave
    for (long base = p0; base < p1; base += CC_TRIP) {
        const long p = base + (long)threadIdx.x * 4;
        i32x4 c = i32x4{0, 0, 0, 0};
        if (p < p1) c = *reinterpret_cast<const i32x4*>(cp + p);
#pragma unroll
        for (int j = 0; j < 4; ++j) if (c[j] < 0 || c[j] > g.L) c[j] = 0;      // not a comp of this shape: never an index
        const int dom = __builtin_amdgcn_readfirstlane(c[0]);
        int dom_count = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) dom_count += __popcll(__ballot(c[j] == dom));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c[j] == dom || c[j] == 0) continue;
            if (c[j] == run_c) { ++run_len; continue; }
            if (run_len) atomicAdd(ar + run_c - 1, run_len);
            run_c = c[j]; run_len = 1;
        }
        if (lane == 0 && dom != 0) atomicAdd(ar + dom - 1, dom_count);
    }
    if (run_len) atomicAdd(ar + run_c - 1, run_len);
}

// A root pixel holds comp == its own index + 1.  PASS 0: the qualifying roots of the chunk are counted into tab (and, in
// LARGEST mode, every root offers its (area, inverted root) key to its value's winner word).  PASS 1 (SPLIT, after the fold
// has turned the chunk counts into their exclusive scan): the root at raster rank r among the image's qualifying roots gets
// label r + 1 if r < max_objects, else 0, written over area[root] - which this thread alone reads in this launch.
template <int PASS, bool LARGEST>
__global__ __launch_bounds__(CC_THREADS) void cc_roots_kernel(const uint8_t* map, const int* comp, CcGeom g, int min_area,
                                                              int max_objects, int* area, int* tabs) {
    __shared__ int sh[CC_THREADS / 64];
    const int s = blockIdx.x, b = blockIdx.y;
    const long p0 = (long)s * g.chunk, p1 = min(g.L, p0 + g.chunk);
    const int* cp = comp + (long)b * g.L;
    const uint8_t* mp = map + (long)b * g.L;
    int* ar = area + (long)b * g.L;
    int* tab = tabs + (long)b * CC_TAB_WORDS;
    int before = PASS == 1 ? tab[CC_TAB_CHUNK + s] : 0;          // qualifying roots of the image ahead of this trip
    int mine = 0;
    for (long base = p0; base < p1; base += CC_TRIP) {           // workgroup-uniform: block_excl_scan holds barriers
        const long p = base + (long)threadIdx.x * 4;
        bool q[4] = {false, false, false, false};
        bool root[4] = {false, false, false, false};
        int cnt = 0;
        if (p < p1) {
            const i32x4 c = *reinterpret_cast<const i32x4*>(cp + p);
            if (c[0] == (int)p + 1 || c[1] == (int)p + 2 || c[2] == (int)p + 3 || c[3] == (int)p + 4) {
                const i32x4 a = *reinterpret_cast<const i32x4*>(ar + p);
                uint32_t mv = 0;
                if constexpr (LARGEST) mv = *reinterpret_cast<const uint32_t*>(mp + p);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    root[j] = c[j] == (int)p + j + 1;
                    q[j] = root[j] && a[j] >= min_area;
                    cnt += q[j];
                    if constexpr (LARGEST) {
                        if (root[j]) {
                            const unsigned long long key = ((unsigned long long)(uint32_t)a[j] << 32) |
                                                           (uint32_t)(0x7fffffff - ((int)p + j));
                            atomicMax(reinterpret_cast<unsigned long long*>(tab + CC_TAB_KEY) + ((mv >> (8 * j)) & 0xffu), key);
                        }
                    }
                }
            }
        }
        if constexpr (PASS == 0) {
            mine += cnt;
        } else {
            int total;
            int r = before + block_excl_scan<CC_THREADS>(cnt, sh, total);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!root[j]) continue;
                int lab = 0;
                if (q[j]) { lab = r < max_objects ? r + 1 : 0; ++r; }
                ar[p + j] = lab;
            }
            before += total;
        }
    }
    if constexpr (PASS == 0) {
        int total;
        block_excl_scan<CC_THREADS>(mine, sh, total);
        if (threadIdx.x == 0) tab[CC_TAB_CHUNK + s] = total;
    }
}

// SPLIT fold: one wave per image over its S <= 64 chunk counts -> their exclusive scan in place, count, dropped
__global__ __launch_bounds__(CC_THREADS) void cc_split_fold_kernel(int* tabs, int S, int n, int max_objects, int* count,
                                                                   int* dropped) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = wave; b < n; b += CC_THREADS / 64) {            // wave-uniform
        int* ch = tabs + (long)b * CC_TAB_WORDS + CC_TAB_CHUNK;
        const int v = lane < S ? ch[lane] : 0;
        const int inc = wave_incl_scan(v);
        if (lane < S) ch[lane] = inc - v;
        const int total = __shfl(inc, 63, 64);
        if (lane == 0) {
            const int given = total < max_objects ? total : max_objects;
            count[b] = given;
            dropped[b] = total - given;
        }
    }
}

// LARGEST fold: one workgroup per image, thread v speaks for input value v
__global__ __launch_bounds__(CC_THREADS) void cc_largest_fold_kernel(int* tabs, int S, int min_area, int max_objects,
                                                                     int* count, int* dropped) {
    __shared__ int sh[CC_THREADS / 64];
    const int b = blockIdx.x, v = threadIdx.x;                   // CC_THREADS == 256 values
    int* tab = tabs + (long)b * CC_TAB_WORDS;
    const unsigned long long key = reinterpret_cast<const unsigned long long*>(tab + CC_TAB_KEY)[v];
    const int area = (int)(key >> 32), root = 0x7fffffff - (int)(uint32_t)key;
    const int survives = v > 0 && area >= min_area;              // min_area >= 1 here: a value without pixels has key 0
    int survivors;
    const int rank = block_excl_scan<CC_THREADS>(survives, sh, survivors);
    const int lab = survives && rank < max_objects ? rank + 1 : 0;
    tab[CC_TAB_ROOT + v] = lab ? root + 1 : 0;
    tab[CC_TAB_LAB + v] = lab;
    if (v == 0) {
        int qualifying = 0;
        for (int s = 0; s < S; ++s) qualifying += tab[CC_TAB_CHUNK + s];
        const int given = survivors < max_objects ? survivors : max_objects;
        count[b] = given;
        dropped[b] = qualifying - given;
    }
}

// out = the label of the pixel's component: SPLIT reads it from area[root], LARGEST from the value's table entry
template <bool LARGEST>
__global__ __launch_bounds__(CC_THREADS) void cc_write_kernel(const uint8_t* map, const int* comp, CcGeom g, const int* area,
                                                              const int* tabs, uint8_t* out) {
    __shared__ int win_root[256], win_lab[256];
    const int s = blockIdx.x, b = blockIdx.y;
    if constexpr (LARGEST) {
        const int* tab = tabs + (long)b * CC_TAB_WORDS;
        win_root[threadIdx.x] = tab[CC_TAB_ROOT + threadIdx.x];
        win_lab[threadIdx.x] = tab[CC_TAB_LAB + threadIdx.x];
        __syncthreads();
    }
    const long p0 = (long)s * g.chunk, p1 = min(g.L, p0 + g.chunk);
    const int* cp = comp + (long)b * g.L;
    const int* ar = area + (long)b * g.L;
    for (long p = p0 + (long)threadIdx.x * 4; p < p1; p += CC_TRIP) {
        const i32x4 c = *reinterpret_cast<const i32x4*>(cp + p);
        uint32_t o = 0;
        if (c[0] | c[1] | c[2] | c[3]) {
            uint32_t mv = 0;
            if constexpr (LARGEST) mv = *reinterpret_cast<const uint32_t*>(map + (long)b * g.L + p);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (c[j] <= 0 || c[j] > g.L) continue;
                int lab;
                if constexpr (LARGEST) {
                    const int v = (mv >> (8 * j)) & 0xffu;
                    lab = win_root[v] == c[j] ? win_lab[v] : 0;
                } else {
                    lab = ar[c[j] - 1];
                }
                o |= (uint32_t)lab << (8 * j);
            }
        }
        *reinterpret_cast<uint32_t*>(out + (long)b * g.L + p) = o;
    }
}

bool cc_shape_ok(int n, int h, int w) {
    return n > 0 && n <= 65535 && h > 0 && w > 0 && w % 4 == 0 && (int64_t)h * w < (1L << 30);
}

}  // namespace

extern "C" int isa_cc_label(const uint8_t* map, int32_t n, int32_t h, int32_t w, int32_t connectivity, int32_t* comp,
                            int32_t* n_comp, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!map || !comp || !n_comp || !scratch || !cc_shape_ok(n, h, w) || (connectivity != 4 && connectivity != 8))
        return ISA_EINVAL;
    if (!aligned(map, 4) || !aligned(comp, 16) || !aligned(n_comp, 4) || !aligned(scratch, 16)) return ISA_EALIGN;
    if (scratch_bytes < ISA_CC_LABEL_SCRATCH_BYTES(n, h, w)) return ISA_ENOMEM;
    const long hw = (long)h * w;
    int* parent = reinterpret_cast<int*>(scratch);
    hipStream_t st = as_stream(stream);
    const dim3 block(CC_THREADS);
    const int tiles_x = cdiv(w, CC_TW);
    const dim3 tiles(tiles_x * cdiv(h, CC_TH), n);           // < 2^30 / 2048 * 64 tiles
    const int row_items = (h - 1) / CC_TH * w, items = row_items + (w - 1) / CC_TW * h;      // < 2^30 / 16
    if (connectivity == 8) {
        hipLaunchKernelGGL(cc_tile_kernel<true>, tiles, block, 0, st, map, h, w, tiles_x, parent, n_comp);
        if (items) hipLaunchKernelGGL(cc_merge_kernel<true>, dim3(cdiv(items, CC_THREADS), n), block, 0, st, map, h, w,
                                      row_items, items, parent);
    } else {
        hipLaunchKernelGGL(cc_tile_kernel<false>, tiles, block, 0, st, map, h, w, tiles_x, parent, n_comp);
        if (items) hipLaunchKernelGGL(cc_merge_kernel<false>, dim3(cdiv(items, CC_THREADS), n), block, 0, st, map, h, w,
                                      row_items, items, parent);
    }
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(cdiv(hw, CC_THREADS * 4), n), block, 0, st, parent, hw, comp, n_comp);
    return launch_status();
}

extern "C" int isa_cc_select(const uint8_t* map, const int32_t* comp, int32_t n, int32_t h, int32_t w, int32_t mode,
                             int32_t min_area, int32_t max_objects, uint8_t* out, int32_t* count, int32_t* dropped,
                             void* scratch, int64_t scratch_bytes, void* stream) {
    if (!map || !comp || !out || !count || !dropped || !scratch || !cc_shape_ok(n, h, w) ||
        (mode != ISA_CC_SPLIT && mode != ISA_CC_LARGEST) || max_objects < 1 || max_objects > 255)
        return ISA_EINVAL;
    const long hw = (long)h * w;
    if (ranges_overlap(out, (uintptr_t)n * hw, map, (uintptr_t)n * hw)) return ISA_EINVAL;   // out may not alias map
    if (!aligned(map, 4) || !aligned(comp, 16) || !aligned(out, 4) || !aligned(count, 4) ||
        !aligned(dropped, 4) || !aligned(scratch, 16))
        return ISA_EALIGN;
    if (scratch_bytes < ISA_CC_SELECT_SCRATCH_BYTES(n, h, w)) return ISA_ENOMEM;
    if (min_area < 1) min_area = 1;
    int* area = reinterpret_cast<int*>(scratch);
    int* tabs = area + (long)n * hw;                             // 16-byte aligned: hw % 4 == 0
    const CcGeom g = cc_geom(hw);
    hipStream_t st = as_stream(stream);
    const dim3 grid(g.S, n), block(CC_THREADS);
    const long vecs = (long)(ISA_CC_SELECT_SCRATCH_BYTES(n, h, w) / 16);
    hipLaunchKernelGGL(cc_clear_kernel, dim3(grid_cap(cdiv(vecs, CC_THREADS))), block, 0, st, reinterpret_cast<i32x4*>(scratch),
                       vecs);
    hipLaunchKernelGGL(cc_area_kernel, grid, block, 0, st, comp, g, area);
    if (mode == ISA_CC_SPLIT) {
        hipLaunchKernelGGL((cc_roots_kernel<0, false>), grid, block, 0, st, map, comp, g, min_area, max_objects, area, tabs);
        hipLaunchKernelGGL(cc_split_fold_kernel, dim3(1), block, 0, st, tabs, g.S, n, max_objects, count, dropped);
        hipLaunchKernelGGL((cc_roots_kernel<1, false>), grid, block, 0, st, map, comp, g, min_area, max_objects, area, tabs);
        hipLaunchKernelGGL(cc_write_kernel<false>, grid, block, 0, st, map, comp, g, area, tabs, out);
    } else {
        hipLaunchKernelGGL((cc_roots_kernel<0, true>), grid, block, 0, st, map, comp, g, min_area, max_objects, area, tabs);
        hipLaunchKernelGGL(cc_largest_fold_kernel, dim3(n), block, 0, st, tabs, g.S, min_area, max_objects, count, dropped);
        hipLaunchKernelGGL(cc_write_kernel<true>, grid, block, 0, st, map, comp, g, area, tabs, out);
    }
    return launch_status();
}
