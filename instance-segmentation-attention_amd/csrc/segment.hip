// Ground-truth-free instance inference (ReSeg.segment): the two per-iteration steps that are not the decoder pass.
//
// The loop keeps, per image, a uint8 label map and the set `remaining` = foreground pixels that carry label 0.  An
// iteration picks the glimpse point s_t = first arg-max of the hard-attention score map `merge` over `remaining`, runs
// the five-level decoder on it, and the instance claims every remaining pixel the level-4 prediction calls foreground
// (l1 > l0), plus the point itself.  Here:
//   isa_seg_begin: labels = 0, count = 0, first point and `active` flag per image, "any image active" word;
//   isa_seg_claim: ONE pass over [n, L] that writes the labels of the claimed pixels and, in the same pass, finds the
//                  NEXT iteration's point over what stays remaining.
// A row (65 536 pixels at 256 x 256) is cut into S <= ISA_ROW_CHUNKS chunks, one 256-thread workgroup each (16 rows on
// 256 CUs otherwise); every workgroup leaves one candidate {score, pixel} in part[b][s], and a second tiny launch folds
// the S candidates of every row: larger score wins, equal scores go to the smaller pixel index, whatever order the
// workgroups ran in.  The fold is also the only writer of count / active / s_next, which the chunk pass only reads.
// Arg-max rules: NaN scores count as -inf (they never beat a number); if no remaining pixel has a score above -inf the
// first remaining pixel is the point, so the point is always a remaining pixel and every iteration claims at least it.
#include "common.hpp"

namespace {

constexpr int SEG_THREADS = 256, SEG_VEC = 4, SEG_TRIP = SEG_THREADS * SEG_VEC;
constexpr int SEG_MIN_CHUNK = 4096;
constexpr int SEG_NONE = 0x7fffffff;        // candidate index of "no remaining pixel"
constexpr int SEG_MAX_LABEL = 255;          // labels are uint8

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct Cand { float v; int i; };

// is b the better candidate?  (scores are NaN-free here)
__device__ __forceinline__ bool cand_better(const Cand& a, const Cand& b) {
    return b.i != SEG_NONE && (a.i == SEG_NONE || b.v > a.v || (b.v == a.v && b.i < a.i));
}
// a thread meets its pixels in increasing order: a later pixel must be strictly larger to replace the candidate
__device__ __forceinline__ void cand_visit(Cand& c, float v, int p) {
    v = v != v ? -INFINITY : v;
    if (c.i == SEG_NONE || v > c.v) { c.v = v; c.i = p; }
}
__device__ __forceinline__ Cand wave_cand(Cand c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Cand t{__shfl_xor(c.v, o, 64), __shfl_xor(c.i, o, 64)};
        if (cand_better(c, t)) c = t;
    }
    return c;
}
// candidate of the whole workgroup in thread 0
__device__ __forceinline__ Cand block_cand(Cand c, float* shv, int* shi) {
    c = wave_cand(c);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { shv[wave] = c.v; shi[wave] = c.i; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < SEG_THREADS / 64; ++w) {
            Cand t{shv[w], shi[w]};
            if (cand_better(c, t)) c = t;
        }
    return c;
}
__device__ __forceinline__ void part_store(float* part, int S, int b, int s, const Cand& c) {
    float* pt = part + ((long)b * S + s) * 2;
    pt[0] = c.v; pt[1] = __int_as_float(c.i);
}

struct SegGeom { long L; int S; long chunk; };      // chunk: pixels per workgroup, a multiple of SEG_TRIP

// ---- isa_seg_begin, chunk pass: labels = 0, candidate over the foreground ------------------------------------------
__global__ __launch_bounds__(SEG_THREADS) void seg_begin_kernel(const float* sem, const float* merge, SegGeom g,
                                                                uint8_t* labels, float* part) {
    __shared__ float shv[SEG_THREADS / 64];
    __shared__ int shi[SEG_THREADS / 64];
    const int s = blockIdx.x, b = blockIdx.y;
    const long p0 = (long)s * g.chunk, p1 = min(g.L, p0 + g.chunk);
    const float* fg = sem + (long)b * g.L; const float* mg = merge + (long)b * g.L;
    uint8_t* lab = labels + (long)b * g.L;
    Cand c{-INFINITY, SEG_NONE};
    for (long p = p0 + (long)threadIdx.x * SEG_VEC; p < p1; p += SEG_TRIP) {
        const f32x4 f = *reinterpret_cast<const f32x4*>(fg + p);
        *reinterpret_cast<uint32_t*>(lab + p) = 0u;
        if (f[0] > 0.5f || f[1] > 0.5f || f[2] > 0.5f || f[3] > 0.5f) {
            const f32x4 m = *reinterpret_cast<const f32x4*>(mg + p);
#pragma unroll
            for (int j = 0; j < SEG_VEC; ++j) if (f[j] > 0.5f) cand_visit(c, m[j], (int)p + j);
        }
    }
    c = block_cand(c, shv, shi);
    if (threadIdx.x == 0) part_store(part, g.S, b, s, c);
}

// ---- isa_seg_claim, chunk pass --------------------------------------------------------------------------------------
// the two logits of 4 consecutive pixels; PACKED: ld == 2, the 8 values are contiguous (16-byte loads)
template <typename T, bool PACKED>
__device__ __forceinline__ void load_pairs(const T* q, int ld, float (&l0)[SEG_VEC], float (&l1)[SEG_VEC]) {
    if constexpr (PACKED) {
        float v[8];
        load8<T>(q, v);
#pragma unroll
        for (int j = 0; j < SEG_VEC; ++j) { l0[j] = v[2 * j]; l1[j] = v[2 * j + 1]; }
    } else {
#pragma unroll
        for (int j = 0; j < SEG_VEC; ++j) {
            if constexpr (sizeof(T) == 4) {
                const f32x2 t = *reinterpret_cast<const f32x2*>(q + (long)j * ld);
                l0[j] = t[0]; l1[j] = t[1];
            } else {
                const bf16x2 t = *reinterpret_cast<const bf16x2*>(q + (long)j * ld);
                l0[j] = (float)t[0]; l1[j] = (float)t[1];
            }
        }
    }
}

template <typename T, bool PACKED>
__global__ __launch_bounds__(SEG_THREADS) void seg_claim_kernel(const T* pred, int ld, const float* sem, const float* merge,
                                                                const int32_t* s_t, const int32_t* count,
                                                                const int32_t* active, SegGeom g, uint8_t* labels,
                                                                float* part) {
    __shared__ float shv[SEG_THREADS / 64];
    __shared__ int shi[SEG_THREADS / 64];
    const int s = blockIdx.x, b = blockIdx.y;
    const long p0 = (long)s * g.chunk, p1 = min(g.L, p0 + g.chunk);
    const float* fg = sem + (long)b * g.L; const float* mg = merge + (long)b * g.L;
    uint8_t* lab = labels + (long)b * g.L;
    const T* pr = pred + (long)b * g.L * ld;
    const int cnt = count[b];
    const bool act = active[b] != 0 && cnt < SEG_MAX_LABEL;
    const uint32_t mine = (uint32_t)(cnt + 1);
    const int sp = s_t[b];
    Cand c{-INFINITY, SEG_NONE};
    for (long p = p0 + (long)threadIdx.x * SEG_VEC; p < p1; p += SEG_TRIP) {
        const f32x4 f = *reinterpret_cast<const f32x4*>(fg + p);
        const uint32_t lv = *reinterpret_cast<const uint32_t*>(lab + p);
        bool rem[SEG_VEC];
        bool any = false;
#pragma unroll
        for (int j = 0; j < SEG_VEC; ++j) { rem[j] = f[j] > 0.5f && ((lv >> (8 * j)) & 0xffu) == 0u; any |= rem[j]; }
        if (!any) continue;                      // background, or claimed by an earlier instance: nothing to read
        const f32x4 m = *reinterpret_cast<const f32x4*>(mg + p);
        if (act) {
            float l0[SEG_VEC], l1[SEG_VEC];
            load_pairs<T, PACKED>(pr + p * ld, ld, l0, l1);
            uint32_t nv = lv;
#pragma unroll
            for (int j = 0; j < SEG_VEC; ++j)
                if (rem[j] && (l1[j] > l0[j] || (int)p + j == sp)) { nv |= mine << (8 * j); rem[j] = false; }
            if (nv != lv) *reinterpret_cast<uint32_t*>(lab + p) = nv;
        }
#pragma unroll
        for (int j = 0; j < SEG_VEC; ++j) if (rem[j]) cand_visit(c, m[j], (int)p + j);
    }
    c = block_cand(c, shv, shi);
    if (threadIdx.x == 0) part_store(part, g.S, b, s, c);
}

// ---- the fold: one wave per row over its S <= 64 chunk candidates; the only writer of count / active / s_next ------
__global__ __launch_bounds__(SEG_THREADS) void seg_fold_kernel(const float* part, int S, int n, int begin, int32_t* count,
                                                               int32_t* active, int32_t* s_next, int32_t* any_active) {
    __shared__ int sh_any[SEG_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int any = 0;
    for (int b = wave; b < n; b += SEG_THREADS / 64) {
        Cand c{-INFINITY, SEG_NONE};
        if (lane < S) { const float* pt = part + ((long)b * S + lane) * 2; c.v = pt[0]; c.i = __float_as_int(pt[1]); }
        c = wave_cand(c);
        if (lane == 0) {
            const int cnt = begin ? 0 : count[b];
            const int claimed = (!begin && active[b] != 0 && cnt < SEG_MAX_LABEL) ? 1 : 0;
            count[b] = cnt + claimed;
            active[b] = c.i != SEG_NONE ? 1 : 0;
            s_next[b] = c.i != SEG_NONE ? c.i : 0;
        }
        any |= c.i != SEG_NONE ? 1 : 0;
    }
    if (lane == 0) sh_any[wave] = any;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SEG_THREADS / 64; ++w) any |= sh_any[w];
        any_active[0] = any;
    }
}

bool seg_geom(int64_t L, SegGeom* g) {
    if (L <= 0 || L % SEG_VEC || L > 0x7fffffffL - SEG_TRIP) return false;
    long S = (L + SEG_MIN_CHUNK - 1) / SEG_MIN_CHUNK;
    if (S > ISA_ROW_CHUNKS) S = ISA_ROW_CHUNKS;
    long chunk = (L + S - 1) / S;
    chunk = (chunk + SEG_TRIP - 1) / SEG_TRIP * SEG_TRIP;
    S = (L + chunk - 1) / chunk;
    *g = SegGeom{(long)L, (int)S, chunk};
    return true;
}

}  // namespace

extern "C" int isa_seg_begin(const float* sem, const float* merge, int32_t n, int64_t L, uint8_t* labels, int32_t* count,
                             int32_t* s_t, int32_t* active, int32_t* any_active, float* part, void* stream) {
    SegGeom g;
    if (!sem || !merge || !labels || !count || !s_t || !active || !any_active || !part || n <= 0 || n > 65535 ||
        !seg_geom(L, &g))
        return ISA_EINVAL;
    if (!aligned(sem, 16) || !aligned(merge, 16) || !aligned(labels, 4)) return ISA_EALIGN;
    hipLaunchKernelGGL(seg_begin_kernel, dim3(g.S, n), dim3(SEG_THREADS), 0, as_stream(stream), sem, merge, g, labels, part);
    hipLaunchKernelGGL(seg_fold_kernel, dim3(1), dim3(SEG_THREADS), 0, as_stream(stream), part, g.S, n, 1, count, active,
                       s_t, any_active);
    return launch_status();
}

extern "C" int isa_seg_claim(const isa_tensor* pred, const float* sem, const float* merge, const int32_t* s_t,
                             uint8_t* labels, int32_t* count, int32_t* active, int32_t* s_next, int32_t* any_active,
                             float* part, void* stream) {
    SegGeom g;
    if (!tensor_ok(pred, 2) || pred->c != 2 || pred->n > 65535 || !sem || !merge || !s_t || !labels || !count || !active ||
        !s_next || !any_active || !part || !seg_geom((int64_t)pred->h * pred->w, &g))
        return ISA_EINVAL;
    if (!aligned(sem, 16) || !aligned(merge, 16) || !aligned(labels, 4)) return ISA_EALIGN;
    const int n = pred->n, ld = pred->ld;
    const bool packed = ld == 2 && aligned(pred->data, 16);
    const dim3 grid(g.S, n), block(SEG_THREADS);
    hipStream_t st = as_stream(stream);
    by_dtype(pred->dtype, [&](auto t) { by_flag(packed, [&](auto pk) {
        hipLaunchKernelGGL((seg_claim_kernel<decltype(t), decltype(pk)::value>), grid, block, 0, st, reinterpret_cast<const decltype(t)*>(pred->data),
                           ld, sem, merge, s_t, count, active, g, labels, part);
    }); });
    hipLaunchKernelGGL(seg_fold_kernel, dim3(1), dim3(SEG_THREADS), 0, st, part, g.S, n, 0, count, active, s_next, any_active);
    return launch_status();
}
