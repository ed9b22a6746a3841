// Exact Euclidean distance transform of uint8 label maps to the two nearest instances, and the two small kernels built on it.
//   isa_edt2_u8       : labels uint8 [n,h,w] -> d1sq, d2sq int32 [n,h,w] (squared distance to the nearest and the second-nearest
//                       label) and nearest uint8 [n,h,w] (the smallest label at distance d1sq);
//   isa_border_weights: the U-Net border weight map 1 + w0 * exp(-(d1 + d2)^2 / (2 sigma^2)) on unlabelled pixels;
//   isa_fill_labels   : every unlabelled foreground pixel takes its nearest label (a Voronoi fill), with a count per image.
// With D_k(p) the squared distance from p to the nearest pixel of label k, d1sq = min_k D_k and d2sq = min_{k != nearest} D_k.
// The transform is separable, in two launches, neither of which waits for another workgroup:
//   1 columns: one lane per column sweeps it down and up and leaves two entries per pixel in `scratch`, packed as
//            (vertical distance << 8 | label), so an unsigned compare orders them by (distance, label):
//              A = the nearest labelled pixel of the column (an up/down tie goes to the smaller label),
//              B = the nearest labelled pixel of the column whose label is not A's.
//   2 rows:  one workgroup per row stages the row's entries in LDS; the lane that owns x walks x' = x, x-1, x+1, x-2, ..
//            and keeps the least (dx^2 + g^2, label) and the least distance among candidates of another label.
// The two entries are enough.  Let L be the nearest label of p and k != L the label of the second-nearest instance, reached
// through column x' at vertical distance g_k.  If neither A(x') nor B(x') is of label k, both are at most g_k away and of
// two different labels, so one of them is not L and gives a candidate of another label that is no farther: the value of
// d2sq is the same.  For d1sq the nearest labelled pixel of every column is A.
// The walk stops at the first dx with dx^2 > d2sq (nothing farther can change either result; a candidate AT d1sq can
// still lower `nearest`, and d1sq <= d2sq).  While no second label has been met d2sq is the sentinel and the walk goes on
// to both ends of the row, so a single distant instance is always reached - except when the row's entries hold one label
// only, which means the whole image does (an entry exists for every column that holds a label): then d2sq is the sentinel
// for good and the walk stops on d1sq instead.
// Everything is an integer and no atomic decides anything: the result is unique and two runs are bit-identical.
#include "common.hpp"

namespace {

constexpr int EDT_COL_THREADS = ISA_EDT_COL_LANES;   // columns per workgroup of the column pass: one wave
constexpr int EDT_ROWS = 8;                          // rows a lane loads ahead of the sweep (independent loads in flight)
constexpr int EDT_ROW_THREADS = ISA_EDT_ROW_LANES;   // lanes of a row workgroup at most (fewer when w is smaller)
constexpr uint32_t EDT_NONE = 0xffffffffu;           // no such pixel in the column
constexpr int EDT_INF = 0x7fffffff;
constexpr int DT_THREADS = 256;

typedef int i32x4 __attribute__((ext_vector_type(4)));


// the last labelled pixel met by a sweep (a) and the last one met whose label is not a's (b); label 0 = none yet
struct Sweep {
    int ya, la, yb, lb;
    __device__ __forceinline__ void init() { ya = 0; la = 0; yb = 0; lb = 0; }
    __device__ __forceinline__ void see(int y, int l) {
        if (l == 0) return;
        if (l != la) { yb = ya; lb = la; la = l; }               // the pixel just left is the nearest one of another label
        ya = y;
    }
    __device__ __forceinline__ uint32_t a(int y) const { return la ? ((uint32_t)abs(y - ya) << 8) | (uint32_t)la : EDT_NONE; }
    __device__ __forceinline__ uint32_t b(int y) const { return lb ? ((uint32_t)abs(y - yb) << 8) | (uint32_t)lb : EDT_NONE; }
};

// ---- launch 1: the columns ---------------------------------------------------------------------------------------------------
// ent[y][x] = {A, B}.  The sweep down leaves the entries seen from above; the sweep up reads them back (the lane's own
// stores: no other lane touches its column), joins them with what it sees from below and writes the final pair.
__global__ __launch_bounds__(EDT_COL_THREADS) void edt_columns_kernel(const uint8_t* labels, int h, int w, uint2* ent) {
    const int x = blockIdx.x * EDT_COL_THREADS + threadIdx.x;
    if (x >= w) return;
    const long hw = (long)h * w;
    const uint8_t* m = labels + (long)blockIdx.y * hw + x;
    uint2* e = ent + (long)blockIdx.y * hw + x;
    Sweep s;
    s.init();
    for (int y0 = 0; y0 < h; y0 += EDT_ROWS) {
        int v[EDT_ROWS];
#pragma unroll
        for (int j = 0; j < EDT_ROWS; ++j) v[j] = y0 + j < h ? m[(long)(y0 + j) * w] : 0;
#pragma unroll
        for (int j = 0; j < EDT_ROWS; ++j) {
            const int y = y0 + j;
            if (y >= h) break;
            s.see(y, v[j]);
            e[(long)y * w] = make_uint2(s.a(y), s.b(y));
        }
    }
    s.init();
    for (int y0 = (h - 1) / EDT_ROWS * EDT_ROWS; y0 >= 0; y0 -= EDT_ROWS) {
        int v[EDT_ROWS];
        uint2 up[EDT_ROWS];
#pragma unroll
        for (int j = 0; j < EDT_ROWS; ++j) {
            const bool in = y0 + j < h;
            v[j] = in ? m[(long)(y0 + j) * w] : 0;
            up[j] = in ? e[(long)(y0 + j) * w] : make_uint2(EDT_NONE, EDT_NONE);
        }
#pragma unroll
        for (int j = EDT_ROWS - 1; j >= 0; --j) {
            const int y = y0 + j;
            if (y >= h) continue;
            s.see(y, v[j]);
            const uint32_t c[4] = {up[j].x, s.a(y), up[j].y, s.b(y)};
            const uint32_t best = min(c[0], c[1]);               // (distance, label): a tie in distance goes to the smaller label
            uint32_t second = EDT_NONE;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c[k] != EDT_NONE && ((c[k] ^ best) & 0xffu)) second = min(second, c[k]);
            e[(long)y * w] = make_uint2(best, second);
        }
    }
}

// ---- launch 2: the rows ------------------------------------------------------------------------------------------------------
struct Two {
    int d1, l1, d2;
    __device__ __forceinline__ void offer(uint32_t c, int dx2) {
        if (c == EDT_NONE) return;
        const int g = (int)(c >> 8), l = (int)(c & 0xffu), d = dx2 + g * g;      // <= 2 * 4095^2 < 2^31
        if (d < d1 || (d == d1 && l < l1)) {
            if (l != l1) { d2 = d1; l1 = l; }                    // the old best is the nearest of another label now
            d1 = d;
        } else if (l != l1 && d < d2) {
            d2 = d;
        }
    }
};

// dynamic LDS: uint2 row[w], then int flag[3] = {smallest A label of the row (256: none), largest (0: none), any B entry}
__global__ __launch_bounds__(EDT_ROW_THREADS) void edt_rows_kernel(const uint2* ent, int h, int w, int* d1sq, int* d2sq, uint8_t* nearest) {
    extern __shared__ __attribute__((aligned(16))) uint2 row[];
    int* flag = reinterpret_cast<int*>(row + w);
    const int y = blockIdx.x;
    const long base = ((long)blockIdx.y * h + y) * w;
    if (threadIdx.x == 0) { flag[0] = 256; flag[1] = 0; flag[2] = 0; }
    __syncthreads();
    int lo = 256, hi = 0, any_b = 0;
    for (int x = threadIdx.x; x < w; x += blockDim.x) {
        const uint2 c = ent[base + x];
        row[x] = c;
        if (c.x != EDT_NONE) { lo = min(lo, (int)(c.x & 0xffu)); hi = max(hi, (int)(c.x & 0xffu)); }
        if (c.y != EDT_NONE) any_b = 1;
    }
    if (hi) {                                                    // LDS, integer: the order does not matter
        atomicMin(flag, lo);
        atomicMax(flag + 1, hi);
        if (any_b) atomicOr(flag + 2, 1);
    }
    __syncthreads();
    const bool empty = flag[1] == 0;                             // no label in the image: nothing to walk to
    const bool single = flag[0] == flag[1] && flag[2] == 0;      // one label in the image: d2sq stays the sentinel
    for (int x = threadIdx.x; x < w; x += blockDim.x) {
        Two t;
        t.d1 = EDT_INF; t.l1 = 0; t.d2 = EDT_INF;
        const uint2 c0 = row[x];
        t.offer(c0.x, 0);
        t.offer(c0.y, 0);
        const int reach = empty ? 0 : max(x, w - 1 - x);
        for (int dx = 1; dx <= reach; ++dx) {
            const int dx2 = dx * dx;
            if (dx2 > (single ? t.d1 : t.d2)) break;
            if (x - dx >= 0) { const uint2 c = row[x - dx]; t.offer(c.x, dx2); t.offer(c.y, dx2); }
            if (x + dx < w) { const uint2 c = row[x + dx]; t.offer(c.x, dx2); t.offer(c.y, dx2); }
        }
        if (d1sq) d1sq[base + x] = t.d1;
        if (d2sq) d2sq[base + x] = t.d2;
        if (nearest) nearest[base + x] = (uint8_t)t.l1;
    }
}

// ---- the weight map and the fill: four pixels per lane ---------------------------------------------------------------------------
__global__ __launch_bounds__(DT_THREADS) void border_weights_kernel(const uint8_t* labels, const int* d1sq, const int* d2sq,
                                                                    const float* cfg, long total, float* out) {
    const float w0 = cfg[0], sigma = cfg[1];
    const float inv = 1.f / (2.f * sigma * sigma);
    for (long p = ((long)blockIdx.x * DT_THREADS + threadIdx.x) * 4; p < total; p += (long)gridDim.x * DT_THREADS * 4) {
        const uint32_t lv = *reinterpret_cast<const uint32_t*>(labels + p);
        const i32x4 a = *reinterpret_cast<const i32x4*>(d1sq + p), b = *reinterpret_cast<const i32x4*>(d2sq + p);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = 1.f;
            if (((lv >> (8 * j)) & 0xffu) == 0 && b[j] != EDT_INF) {
                const float s = sqrtf((float)a[j]) + sqrtf((float)b[j]);
                v = 1.f + w0 * expf(-(s * s) * inv);
            }
            o[j] = v;
        }
        *reinterpret_cast<f32x4*>(out + p) = o;
    }
}

__global__ __launch_bounds__(DT_THREADS) void fill_clear_kernel(int* filled, int n) {
    const int i = blockIdx.x * DT_THREADS + threadIdx.x;
    if (i < n) filled[i] = 0;
}

// grid (chunks, n): a workgroup stays inside one image, a wave adds its count once
__global__ __launch_bounds__(DT_THREADS) void fill_labels_kernel(const uint8_t* labels, const uint8_t* fg, const uint8_t* nearest,
                                                                 const int* d1sq, int max_dist_sq, long hw, uint8_t* out,
                                                                 int* filled) {
    const long off = (long)blockIdx.y * hw;
    int cnt = 0;
    for (long p = ((long)blockIdx.x * DT_THREADS + threadIdx.x) * 4; p < hw; p += (long)gridDim.x * DT_THREADS * 4) {
        const uint32_t lv = *reinterpret_cast<const uint32_t*>(labels + off + p);
        uint32_t o = lv;
        if ((lv & 0xffu) == 0 || (lv & 0xff00u) == 0 || (lv & 0xff0000u) == 0 || (lv >> 24) == 0) {
            const uint32_t fv = *reinterpret_cast<const uint32_t*>(fg + off + p);
            const uint32_t nv = *reinterpret_cast<const uint32_t*>(nearest + off + p);
            const i32x4 d = *reinterpret_cast<const i32x4*>(d1sq + off + p);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t near_j = (nv >> (8 * j)) & 0xffu;
                if (((lv >> (8 * j)) & 0xffu) == 0 && ((fv >> (8 * j)) & 0xffu) != 0 && near_j != 0 &&
                    (max_dist_sq < 0 || d[j] <= max_dist_sq)) {
                    o |= near_j << (8 * j);
                    ++cnt;
                }
            }
        }
        *reinterpret_cast<uint32_t*>(out + off + p) = o;
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(filled + blockIdx.y, cnt);
}


}  // namespace

extern "C" int isa_edt2_u8(const uint8_t* labels, int32_t n, int32_t h, int32_t w, int32_t* d1sq, int32_t* d2sq,
                           uint8_t* nearest, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!labels || !scratch || n <= 0 || n > 65535 || h <= 0 || w <= 0 || h > ISA_EDT_MAX_SIDE || w > ISA_EDT_MAX_SIDE ||
        w % 4 != 0)
        return ISA_EINVAL;
    if (!aligned(labels, 4) || !aligned(d1sq, 16) || !aligned(d2sq, 16) || !aligned(nearest, 4) ||
        !aligned(scratch, 16))
        return ISA_EALIGN;
    if (scratch_bytes < ISA_EDT_SCRATCH_BYTES(n, h, w)) return ISA_ENOMEM;
    uint2* ent = reinterpret_cast<uint2*>(scratch);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(edt_columns_kernel, dim3(cdiv(w, EDT_COL_THREADS), n), dim3(EDT_COL_THREADS), 0, st, labels, h, w, ent);
    const int lanes = min(EDT_ROW_THREADS, cdiv(w, 64) * 64);
    hipLaunchKernelGGL(edt_rows_kernel, dim3(h, n), dim3(lanes), (size_t)w * 8 + 16, st, ent, h, w, d1sq, d2sq, nearest);
    return launch_status();
}

extern "C" int isa_border_weights(const uint8_t* labels, const int32_t* d1sq, const int32_t* d2sq, const float* cfg, int32_t n,
                                  int64_t hw, float* out, void* stream) {
    if (!labels || !d1sq || !d2sq || !cfg || !out || n <= 0 || hw <= 0 || hw % 4 != 0 || hw >= (1L << 30)) return ISA_EINVAL;
    if (!aligned(labels, 4) || !aligned(d1sq, 16) || !aligned(d2sq, 16) || !aligned(cfg, 4) || !aligned(out, 16))
        return ISA_EALIGN;
    const long total = (long)n * hw;
    hipLaunchKernelGGL(border_weights_kernel, dim3(grid_cap(cdiv(total, DT_THREADS * 4))), dim3(DT_THREADS), 0,
                       as_stream(stream), labels, d1sq, d2sq, cfg, total, out);
    return launch_status();
}

extern "C" int isa_fill_labels(const uint8_t* labels, const uint8_t* fg, const uint8_t* nearest, const int32_t* d1sq,
                               int32_t max_dist_sq, int32_t n, int64_t hw, uint8_t* out, int32_t* filled, void* stream) {
    if (!labels || !fg || !nearest || !d1sq || !out || !filled || n <= 0 || n > 65535 || hw <= 0 || hw % 4 != 0 ||
        hw >= (1L << 30))
        return ISA_EINVAL;
    if (ranges_overlap(out, (uintptr_t)n * hw, labels, (uintptr_t)n * hw)) return ISA_EINVAL;   // out may not alias labels
    if (!aligned(labels, 4) || !aligned(fg, 4) || !aligned(nearest, 4) || !aligned(d1sq, 16) || !aligned(out, 4) ||
        !aligned(filled, 4))
        return ISA_EALIGN;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(fill_clear_kernel, dim3(cdiv(n, DT_THREADS)), dim3(DT_THREADS), 0, st, filled, (int)n);
    hipLaunchKernelGGL(fill_labels_kernel, dim3(grid_cap(cdiv(hw, DT_THREADS * 4), 64), n), dim3(DT_THREADS), 0, st, labels, fg,
                       nearest, d1sq, max_dist_sq, (long)hw, out, filled);
    return launch_status();
}
