// Tracing the outlines of a uint8 label map on the device: every contour (outer boundary or hole) of every label as a
// polygon of corner points, with its crack length and signed area, in ascending order of start key; and per label the
// number of outer contours, of holes, and the Euler number.  The definitions are in include/isa_kernels.h.
//   isa_contour_trace    : table, verts, counts from the map; 2 R + 9 launches, R = ceil(log4(4 h w));
//   isa_contour_topology : topo from table and counts; one launch.
// A grid point (x0, y0) of the (h+1) x (w+1) lattice sees four pixels, a b above and c d below it, and up to four edges
// start there (E along the top of d, S along the right of c, W along the bottom of a, N along the left of b): the edges
// of an image in ascending key order are the lattice points in raster order, each with its directions in order.
//   1. count_kernel / scan_blocks_kernel / emit_kernel: edges per block of CT_BLOCK points, an exclusive scan of the block
//      sums per image, then base[point] = index of the point's first edge and key[index] for every edge: the compacted
//      index of an edge IS its rank by key, so "smallest key" below is "smallest index".
//   2. succ_kernel: the successor of edge e from the four pixels around its end point P: index = base[P] + the number
//      of P's edges with a smaller direction.  It is a bijection, so thread e may write the corner flag OF ITS SUCCESSOR
//      (successor direction != own direction) without a race.
//   3. min_round_kernel x R: pointer jumping, (next, smallest corner index seen) -> after R rounds the smallest corner
//      index of the whole cycle, the contour's start edge.  A round takes CT_HOPS = 3 hops through the records of the
//      round before, so an edge's record covers four times as many edges after it: half the launches of plain doubling
//      for two more dependent loads each, and at a few thousand edges a round is nothing but its launch.  Ping-pong
//      buffers: a round reads one and writes the other.
//   4. rank_init_kernel + rank_round_kernel x R: the cycle is cut in front of its start edge (the edge whose successor is
//      the start gets no successor) and the suffix sums of (corner flag, 1, x0 y1 - x1 y0) are formed the same way: at the
//      start edge they are the vertex count, the edge count and the twice-area; at a corner edge the first of them gives
//      its position among the vertices.  The area terms are added modulo 2^32: partial sums can leave 32 bits, the total
//      (|2 A| <= 2 h w <= 2^25) cannot.
//   5. final_count_kernel / final_scan_kernel / final_write_kernel / verts_kernel: an exclusive scan over the edges in index
//      order of (is a start edge, its vertex count) gives every contour its row and its vertex offset; rows below cmax
//      are written, counts are set, and every corner edge whose contour has a row and fits below vmax writes its point.
// R comes from the edge bound 4 h w, never from the data; every kernel that walks edges reads the image's edge count from
// scratch and does nothing past it.  Nothing but integers; the only scattered writes go to slots that exactly one thread
// owns: two runs are bit-identical.
#include "common.hpp"

namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_ITEMS = 4;                                              // consecutive points / edges per thread in the scans
constexpr int CT_BLOCK = ISA_CONTOUR_BLOCK;
static_assert(CT_BLOCK == CT_THREADS * CT_ITEMS, "scan block");
constexpr int CT_WALK_BLOCKS = 512;                                      // grid.x of the kernels that stride over edges
constexpr int CT_HOPS = 3;                                               // hops per round: a record's reach grows (CT_HOPS + 1)-fold
constexpr uint32_t NIL = 0xffffffffu;
typedef long long i64;

struct CtGeom {
    int h, w, wp;                // wp = w + 1: lattice points per row
    int npts, nbp;               // lattice points, blocks of them
    int emax, nbe;               // edge bound 4 h w, blocks of it
    int pstride, bstride, fstride;   // ints per image of base, the point block sums and the edge block sums
    int cmax, vmax, conn;
};

// the per-call arrays in scratch; [n][emax] unless stated
struct CtBuf {
    uint32_t *key, *succ, *cflag, *start;
    uint4 *x, *y;                // two regions of 16 bytes per edge: the jumping rounds ping-pong between them
    int32_t *base;               // [n][pstride]
    int32_t *bsum;               // [n][bstride]
    int32_t *fsum;               // [n][fstride], two per block
    int32_t *ecount;             // [n][4], edges of the image in [0]
};

// the pixels around lattice point (px, py): a b above, c d below, -1 outside the image; every load is issued, none in a
// branch (an absent pixel reads pixel 0 and is replaced by a select)
struct Quad { int a, b, c, d; };
__device__ __forceinline__ Quad quad_at(const uint8_t* m, int h, int w, int px, int py) {
    const bool up = py > 0, dn = py < h, lf = px > 0, rt = px < w;
    const int ia = (py - 1) * w + px - 1, ic = py * w + px - 1;
    const int va = m[(up && lf) ? ia : 0], vb = m[(up && rt) ? ia + 1 : 0];
    const int vc = m[(dn && lf) ? ic : 0], vd = m[(dn && rt) ? ic + 1 : 0];
    return Quad{(up && lf) ? va : -1, (up && rt) ? vb : -1, (dn && lf) ? vc : -1, (dn && rt) ? vd : -1};
}
// bit dir is set when an edge of direction dir starts at the point
__device__ __forceinline__ int edge_mask(const Quad& q) {
    return (q.d > 0 && q.d != q.b ? 1 : 0) | (q.c > 0 && q.c != q.d ? 2 : 0) | (q.a > 0 && q.a != q.c ? 4 : 0) |
           (q.b > 0 && q.b != q.a ? 8 : 0);
}

// the edge masks of the thread's CT_ITEMS lattice points of block blockIdx.x; returns their edge count
__device__ __forceinline__ int point_masks(const uint8_t* m, const CtGeom& g, int (&mask)[CT_ITEMS]) {
    const int p0 = blockIdx.x * CT_BLOCK + threadIdx.x * CT_ITEMS;
    int py = p0 / g.wp, px = p0 - py * g.wp, cnt = 0;
#pragma unroll
    for (int i = 0; i < CT_ITEMS; ++i) {
        mask[i] = 0;
        if (p0 + i < g.npts) mask[i] = edge_mask(quad_at(m, g.h, g.w, px, py));
        cnt += __popc(mask[i]);
        if (++px == g.wp) { px = 0; ++py; }
    }
    return cnt;
}

__global__ __launch_bounds__(CT_THREADS) void count_kernel(const uint8_t* labels, CtGeom g, CtBuf b) {
    __shared__ int sh[CT_THREADS / 64];
    const int img = blockIdx.y;
    int mask[CT_ITEMS], total;
    const int cnt = point_masks(labels + (long)img * g.h * g.w, g, mask);
    block_excl_scan<CT_THREADS>(cnt, sh, total);
    if (threadIdx.x == 0) b.bsum[(long)img * g.bstride + blockIdx.x] = total;
}

// one workgroup per image: the block sums become block offsets, their total the image's edge count
__global__ __launch_bounds__(CT_THREADS) void scan_blocks_kernel(CtGeom g, CtBuf b) {
    __shared__ int sh[CT_THREADS / 64];
    const int img = blockIdx.x;
    const int edges = block_scan_walk<CT_THREADS>(b.bsum + (long)img * g.bstride, g.nbp, 1, sh);
    if (threadIdx.x == 0) b.ecount[img * 4] = edges;
}

__global__ __launch_bounds__(CT_THREADS) void emit_kernel(const uint8_t* labels, CtGeom g, CtBuf b) {
    __shared__ int sh[CT_THREADS / 64];
    const int img = blockIdx.y;
    int mask[CT_ITEMS], total;
    const int cnt = point_masks(labels + (long)img * g.h * g.w, g, mask);
    int at = b.bsum[(long)img * g.bstride + blockIdx.x] + block_excl_scan<CT_THREADS>(cnt, sh, total);
    const int p0 = blockIdx.x * CT_BLOCK + threadIdx.x * CT_ITEMS;
    int32_t* base = b.base + (long)img * g.pstride;
    uint32_t* key = b.key + (long)img * g.emax;
#pragma unroll
    for (int i = 0; i < CT_ITEMS; ++i) {
        if (p0 + i >= g.npts) break;
        base[p0 + i] = at;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if (mask[i] >> d & 1) key[at++] = (uint32_t)(p0 + i) * 4u + d;      // at most 4 h w edges exist: at < emax
    }
}

struct EdgeAt { int px, py, dir; };
__device__ __forceinline__ EdgeAt edge_at(uint32_t key, int wp) {
    const int pt = (int)(key >> 2), py = pt / wp;
    return EdgeAt{pt - py * wp, py, (int)(key & 3u)};
}
__device__ __forceinline__ int step_x(int dir) { return dir == 0 ? 1 : dir == 2 ? -1 : 0; }
__device__ __forceinline__ int step_y(int dir) { return dir == 1 ? 1 : dir == 3 ? -1 : 0; }

__global__ __launch_bounds__(CT_THREADS) void succ_kernel(const uint8_t* labels, CtGeom g, CtBuf b) {
    const int img = blockIdx.y, E = b.ecount[img * 4];
    const uint8_t* m = labels + (long)img * g.h * g.w;
    const int32_t* base = b.base + (long)img * g.pstride;
    const long eo = (long)img * g.emax;
    uint2* a0 = reinterpret_cast<uint2*>(b.x) + eo;
    for (int e = blockIdx.x * CT_THREADS + threadIdx.x; e < E; e += gridDim.x * CT_THREADS) {
        const EdgeAt ed = edge_at(b.key[eo + e], g.wp);
        const int d = ed.dir;
        // the owner pixel lies right of the edge: E below its start, S left of it, W above left, N above
        const int oy = ed.py - (d >= 2), ox = ed.px - (d == 1 || d == 2);
        const int v = m[oy * g.w + ox];
        const int px = ed.px + step_x(d), py = ed.py + step_y(d);
        const Quad q = quad_at(m, g.h, g.w, px, py);
        // the two pixels ahead of P: (right, left) = (d, b) heading E, (c, d) heading S, (a, c) heading W, (b, a) heading N
        const int right = d == 0 ? q.d : d == 1 ? q.c : d == 2 ? q.a : q.b;
        const int left = d == 0 ? q.b : d == 1 ? q.d : d == 2 ? q.c : q.a;
        const bool R = right == v, Lf = left == v;
        const int turn = g.conn == 8 ? (Lf ? -1 : R ? 0 : 1) : (!R ? 1 : Lf ? -1 : 0);
        const int nd = (d + turn) & 3;
        int s = base[py * g.wp + px] + __popc(edge_mask(q) & ((1 << nd) - 1));
        if (s >= E) s = e;                                               // cannot happen; keeps every index inside the image
        const bool corner = nd != d;
        b.succ[eo + e] = (uint32_t)s;
        a0[e].x = (uint32_t)s;
        b.cflag[eo + s] = corner;                                        // e is the only predecessor of s
        a0[s].y = corner ? (uint32_t)s : NIL;
    }
}

// (next, smallest corner index among the edges covered so far)
__global__ __launch_bounds__(CT_THREADS) void min_round_kernel(CtGeom g, CtBuf b, const uint2* in, uint2* out) {
    const int img = blockIdx.y, E = b.ecount[img * 4];
    in += (long)img * g.emax;
    out += (long)img * g.emax;
    for (int e = blockIdx.x * CT_THREADS + threadIdx.x; e < E; e += gridDim.x * CT_THREADS) {
        uint2 a = in[e];
#pragma unroll
        for (int k = 0; k < CT_HOPS; ++k) {                              // every hop reads the records of the round before
            const uint2 n = in[a.x];
            a = make_uint2(n.x, min(a.y, n.y));
        }
        out[e] = a;
    }
}

// (corner flag, 1, twice-area term, next) with the cycle cut in front of its start edge
__global__ __launch_bounds__(CT_THREADS) void rank_init_kernel(CtGeom g, CtBuf b, const uint2* fin, uint4* out) {
    const int img = blockIdx.y, E = b.ecount[img * 4];
    const long eo = (long)img * g.emax;
    fin += eo;
    out += eo;
    for (int e = blockIdx.x * CT_THREADS + threadIdx.x; e < E; e += gridDim.x * CT_THREADS) {
        const uint32_t s = fin[e].y, nx = b.succ[eo + e];
        const EdgeAt ed = edge_at(b.key[eo + e], g.wp);
        const int x1 = ed.px + step_x(ed.dir), y1 = ed.py + step_y(ed.dir);
        b.start[eo + e] = s;
        out[e] = make_uint4(b.cflag[eo + e], 1u, (uint32_t)(ed.px * y1 - x1 * ed.py), nx == s ? NIL : nx);
    }
}

__global__ __launch_bounds__(CT_THREADS) void rank_round_kernel(CtGeom g, CtBuf b, const uint4* in, uint4* out) {
    const int img = blockIdx.y, E = b.ecount[img * 4];
    in += (long)img * g.emax;
    out += (long)img * g.emax;
    for (int e = blockIdx.x * CT_THREADS + threadIdx.x; e < E; e += gridDim.x * CT_THREADS) {
        uint4 a = in[e];
#pragma unroll
        for (int k = 0; k < CT_HOPS; ++k) {
            if (a.w == NIL) break;                                       // the end of the cut cycle is reached
            const uint4 n = in[a.w];
            a.x += n.x; a.y += n.y; a.z += n.z; a.w = n.w;
        }
        out[e] = a;
    }
}

// (is a start edge, its vertex count) of the thread's CT_ITEMS edges of block blockIdx.x
__device__ __forceinline__ void start_items(const CtGeom& g, const CtBuf& b, const uint4* sums, int img, int E,
                                            int (&is)[CT_ITEMS], int (&nv)[CT_ITEMS]) {
    const long eo = (long)img * g.emax;
    const int e0 = blockIdx.x * CT_BLOCK + threadIdx.x * CT_ITEMS;
#pragma unroll
    for (int i = 0; i < CT_ITEMS; ++i) {
        const int e = e0 + i;
        is[i] = e < E && b.start[eo + e] == (uint32_t)e;
        nv[i] = is[i] ? (int)sums[eo + e].x : 0;
    }
}

__global__ __launch_bounds__(CT_THREADS) void final_count_kernel(CtGeom g, CtBuf b, const uint4* sums) {
    __shared__ int sh[CT_THREADS / 64];
    const int img = blockIdx.y, E = b.ecount[img * 4];
    if ((int)blockIdx.x * CT_BLOCK >= E) return;                         // uniform for the workgroup
    int is[CT_ITEMS], nv[CT_ITEMS], c = 0, v = 0, tc, tv;
    start_items(g, b, sums, img, E, is, nv);
#pragma unroll
    for (int i = 0; i < CT_ITEMS; ++i) { c += is[i]; v += nv[i]; }
    block_excl_scan<CT_THREADS>(c, sh, tc);
    block_excl_scan<CT_THREADS>(v, sh, tv);
    if (threadIdx.x == 0) {
        b.fsum[(long)img * g.fstride + 2 * blockIdx.x] = tc;
        b.fsum[(long)img * g.fstride + 2 * blockIdx.x + 1] = tv;
    }
}

__global__ __launch_bounds__(CT_THREADS) void final_scan_kernel(CtGeom g, CtBuf b, int32_t* counts) {
    __shared__ int sh[CT_THREADS / 64];
    const int img = blockIdx.x, E = b.ecount[img * 4];
    const int nb = (E + CT_BLOCK - 1) / CT_BLOCK;
    int32_t* s = b.fsum + (long)img * g.fstride;                         // (contours, vertices) per block, interleaved
    const int cc = block_scan_walk<CT_THREADS>(s, nb, 2, sh), cv = block_scan_walk<CT_THREADS>(s + 1, nb, 2, sh);
    if (threadIdx.x == 0) {
        int32_t* o = counts + img * 4;
        o[0] = cc; o[1] = cv; o[2] = max(0, cc - g.cmax); o[3] = max(0, cv - g.vmax);
    }
}

// a start edge learns its contour's row and vertex offset (kept in `where` for verts_kernel) and writes the row
__global__ __launch_bounds__(CT_THREADS) void final_write_kernel(const uint8_t* labels, CtGeom g, CtBuf b, const uint4* sums,
                                                                 uint2* where, i64* table) {
    __shared__ int sh[CT_THREADS / 64];
    const int img = blockIdx.y, E = b.ecount[img * 4];
    if ((int)blockIdx.x * CT_BLOCK >= E) return;
    int is[CT_ITEMS], nv[CT_ITEMS], c = 0, v = 0, tc, tv;
    start_items(g, b, sums, img, E, is, nv);
#pragma unroll
    for (int i = 0; i < CT_ITEMS; ++i) { c += is[i]; v += nv[i]; }
    int row = b.fsum[(long)img * g.fstride + 2 * blockIdx.x] + block_excl_scan<CT_THREADS>(c, sh, tc);
    int off = b.fsum[(long)img * g.fstride + 2 * blockIdx.x + 1] + block_excl_scan<CT_THREADS>(v, sh, tv);
    const long eo = (long)img * g.emax;
    const int e0 = blockIdx.x * CT_BLOCK + threadIdx.x * CT_ITEMS;
#pragma unroll
    for (int i = 0; i < CT_ITEMS; ++i) {
        if (!is[i]) continue;
        const int e = e0 + i;
        where[eo + e] = make_uint2((uint32_t)row, (uint32_t)off);
        if (row < g.cmax) {
            const uint32_t key = b.key[eo + e];
            const EdgeAt ed = edge_at(key, g.wp);
            const int pixel = (ed.py - (ed.dir >= 2)) * g.w + ed.px - (ed.dir == 1 || ed.dir == 2);
            const uint4 t = sums[eo + e];
            i64* r = table + ((long)img * g.cmax + row) * 8;
            r[0] = labels[(long)img * g.h * g.w + pixel];
            r[1] = off; r[2] = (i64)t.x; r[3] = (i64)t.y; r[4] = (i64)(int32_t)t.z; r[5] = (i64)key; r[6] = pixel; r[7] = 0;
        }
        ++row;
        off += nv[i];
    }
}

__global__ __launch_bounds__(CT_THREADS) void verts_kernel(CtGeom g, CtBuf b, const uint4* sums, const uint2* where,
                                                           int16_t* verts) {
    const int img = blockIdx.y, E = b.ecount[img * 4];
    const long eo = (long)img * g.emax;
    for (int e = blockIdx.x * CT_THREADS + threadIdx.x; e < E; e += gridDim.x * CT_THREADS) {
        if (!b.cflag[eo + e]) continue;
        const uint32_t s = b.start[eo + e];
        if (s >= (uint32_t)E) continue;                                  // cannot happen: every cycle has a corner
        const uint2 at = where[eo + s];
        const i64 nv = sums[eo + s].x;
        if (at.x >= (uint32_t)g.cmax || (i64)at.y + nv > g.vmax) continue;     // no row, or the contour does not fit whole
        const i64 k = (i64)at.y + nv - (i64)sums[eo + e].x;              // corners from e to the end of the cut cycle, e included
        if (k < at.y || k >= g.vmax) continue;                           // cannot happen: 1 <= the corner's suffix count <= nv
        const EdgeAt ed = edge_at(b.key[eo + e], g.wp);
        *reinterpret_cast<uint32_t*>(verts + ((long)img * g.vmax + k) * 2) = (uint32_t)ed.px | (uint32_t)ed.py << 16;
    }
}

__global__ __launch_bounds__(CT_THREADS) void topology_kernel(const i64* table, const int32_t* counts, int cmax, int nl,
                                                              int32_t* topo) {
    __shared__ int outer[256], holes[256];
    const int img = blockIdx.x, t = threadIdx.x;
    outer[t] = 0;
    holes[t] = 0;
    __syncthreads();
    const int rows = min(counts[img * 4], cmax);
    for (int r = t; r < rows; r += CT_THREADS) {
        const i64* row = table + ((long)img * cmax + r) * 8;
        const i64 v = row[0];
        if (v >= 0 && v < nl) atomicAdd(row[4] > 0 ? &outer[v] : &holes[v], 1);
    }
    __syncthreads();
    if (t < nl) {
        int32_t* o = topo + ((long)img * nl + t) * 3;
        o[0] = outer[t]; o[1] = holes[t]; o[2] = outer[t] - holes[t];
    }
}

}  // namespace

extern "C" int isa_contour_trace(const uint8_t* labels, int32_t n, int32_t h, int32_t w, int32_t connectivity, int32_t cmax,
                                 int32_t vmax, int64_t* table, int16_t* verts, int32_t* counts, void* scratch,
                                 int64_t scratch_bytes, void* stream) {
    if (!labels || !table || !verts || !counts || !scratch || n <= 0 || n > 65535 || h <= 0 || w <= 0 ||
        h > ISA_CONTOUR_MAX_SIDE || w > ISA_CONTOUR_MAX_SIDE || w % 4 || (connectivity != 4 && connectivity != 8) || cmax < 1 ||
        vmax < 1)
        return ISA_EINVAL;
    if (scratch_bytes < ISA_CONTOUR_SCRATCH_BYTES(n, h, w)) return ISA_ENOMEM;
    if (!aligned(labels, 4) || !aligned(table, 8) || !aligned(verts, 4) || !aligned(counts, 4) || !aligned(scratch, 16))
        return ISA_EALIGN;
    CtGeom g;
    g.h = h; g.w = w; g.wp = w + 1;
    g.npts = (h + 1) * (w + 1);
    g.nbp = cdiv(g.npts, CT_BLOCK);
    g.emax = (int)ISA_CONTOUR_EDGES(h, w);
    g.nbe = cdiv(g.emax, CT_BLOCK);
    g.pstride = (int)ISA_CONTOUR_POINTS(h, w);
    g.bstride = (g.pstride / CT_BLOCK + 1) * 4;
    g.fstride = (g.emax / CT_BLOCK + 1) * 4;
    g.cmax = cmax; g.vmax = vmax; g.conn = connectivity;
    // the layout ISA_CONTOUR_SCRATCH_BYTES adds up: every array starts on a 16-byte boundary (emax and pstride % 4 == 0)
    const size_t ne = (size_t)n * g.emax;
    char* p = static_cast<char*>(scratch);
    auto take = [&p](size_t bytes) { char* at = p; p += bytes; return at; };
    CtBuf b;
    b.x = reinterpret_cast<uint4*>(take(ne * 16));
    b.y = reinterpret_cast<uint4*>(take(ne * 16));
    b.key = reinterpret_cast<uint32_t*>(take(ne * 4));
    b.succ = reinterpret_cast<uint32_t*>(take(ne * 4));
    b.cflag = reinterpret_cast<uint32_t*>(take(ne * 4));
    b.start = reinterpret_cast<uint32_t*>(take(ne * 4));
    b.base = reinterpret_cast<int32_t*>(take((size_t)n * g.pstride * 4));
    b.bsum = reinterpret_cast<int32_t*>(take((size_t)n * g.bstride * 4));
    b.fsum = reinterpret_cast<int32_t*>(take((size_t)n * g.fstride * 4));
    b.ecount = reinterpret_cast<int32_t*>(take((size_t)n * 16));
    int rounds = 0;
    for (long reach = 1; reach < g.emax; reach *= CT_HOPS + 1) ++rounds;     // (CT_HOPS + 1)^rounds >= 4 h w >= any cycle

    hipStream_t st = as_stream(stream);
    const dim3 block(CT_THREADS), pts(g.nbp, n), per_image(n), walk(grid_cap(cdiv(g.emax, CT_THREADS), CT_WALK_BLOCKS), n),
        blocks(g.nbe, n);
    hipLaunchKernelGGL(count_kernel, pts, block, 0, st, labels, g, b);
    hipLaunchKernelGGL(scan_blocks_kernel, per_image, block, 0, st, g, b);
    hipLaunchKernelGGL(emit_kernel, pts, block, 0, st, labels, g, b);
    hipLaunchKernelGGL(succ_kernel, walk, block, 0, st, labels, g, b);
    uint4 *cur = b.x, *other = b.y;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(min_round_kernel, walk, block, 0, st, g, b, reinterpret_cast<const uint2*>(cur),
                           reinterpret_cast<uint2*>(other));
        std::swap(cur, other);
    }
    hipLaunchKernelGGL(rank_init_kernel, walk, block, 0, st, g, b, reinterpret_cast<const uint2*>(cur), other);
    std::swap(cur, other);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(rank_round_kernel, walk, block, 0, st, g, b, static_cast<const uint4*>(cur), other);
        std::swap(cur, other);
    }
    // cur: the suffix sums; other is free again and holds (row, vertex offset) of the start edges
    uint2* where = reinterpret_cast<uint2*>(other);
    hipLaunchKernelGGL(final_count_kernel, blocks, block, 0, st, g, b, static_cast<const uint4*>(cur));
    hipLaunchKernelGGL(final_scan_kernel, per_image, block, 0, st, g, b, counts);
    hipLaunchKernelGGL(final_write_kernel, blocks, block, 0, st, labels, g, b, static_cast<const uint4*>(cur), where,
                       reinterpret_cast<i64*>(table));
    hipLaunchKernelGGL(verts_kernel, walk, block, 0, st, g, b, static_cast<const uint4*>(cur), static_cast<const uint2*>(where),
                       verts);
    return launch_status();
}

extern "C" int isa_contour_topology(const int64_t* table, const int32_t* counts, int32_t n, int32_t cmax, int32_t nl,
                                    int32_t* topo, void* stream) {
    if (!table || !counts || !topo || n <= 0 || n > 65535 || cmax < 1 || nl < 1 || nl > 256) return ISA_EINVAL;
    if (!aligned(table, 8) || !aligned(counts, 4) || !aligned(topo, 4)) return ISA_EALIGN;
    hipLaunchKernelGGL(topology_kernel, dim3(n), dim3(CT_THREADS), 0, as_stream(stream), reinterpret_cast<const i64*>(table),
                       counts, cmax, nl, topo);
    return launch_status();
}
