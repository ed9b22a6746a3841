// Copy-paste augmentation (Ghiasi et al., CVPR 2021) on a batch: some instances of another image of the batch, flipped
// and shifted, are pasted over the target; image, semantic map, occluded instance planes and object count are updated
// together.  The contract is in include/isa_kernels.h (isa_copy_paste_u8) and DESIGN.md section 19.
// A fixed sequence on the caller's stream, whatever the data: a small launch that clears the counters and three launches of
// grid (chunks of the image, n) x 256 lanes, a lane per pixel:
//   1 areas:   over the in-frame window of the target, the source pixel's plane vector -> area[b][j];
//   2 apply:   every workgroup derives its image's paste set from the <= 32 area counters (lane 0, through LDS), writes
//              rgb_out and sem_out, the masked target planes at [0, n_b) and the pasted planes at [n_b, n_b + |P|), and
//              counts the non-zero bytes left per target plane -> remain[b][i];
//   3 compact: every workgroup derives the kept set from remain, so the channel map; a workgroup whose image dropped
//              nothing exits at once; otherwise every lane permutes its pixel's plane vector in place (a lane reads and
//              writes one pixel alone: no hazard).  The first workgroup of an image writes n_out and plan.
// A pixel's planes travel as one vector of at most 32 bytes in 8 registers: 16-byte loads and stores when k % 16 == 0,
// bytes otherwise.  "Is this byte non-zero" is byte-parallel (a 32-bit mask per pixel from 8 words); a plane's pixels are
// counted by a ballot and a popcount per wave, lane j keeps plane j's count, the waves fold in LDS and a workgroup adds
// one integer atomic per plane.  Integer atomics commute, so two runs give the same bytes.  No float arithmetic.
#include "common.hpp"

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_PIX_PER_LANE = 4;                   // pixels a lane walks when the image is large enough
constexpr int CP_MAX_CHUNKS = 256;                   // workgroups per image at most

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct CpArgs {
    const uint8_t *rgb, *sem, *planes;
    const int32_t *n_objects, *xform;
    const uint32_t* select;
    int n, h, w, c, k, min_area;
    uint8_t *rgb_out, *sem_out, *planes_out;
    int32_t *n_out, *plan, *area, *remain;
};

// ---- a pixel's plane vector ---------------------------------------------------------------------------------------------
struct PVec { uint32_t w[8]; };

template <bool VEC> __device__ __forceinline__ PVec pv_load(const uint8_t* p, int k) {
    PVec v;
    if constexpr (VEC) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(p);
        u32x4 b = {0u, 0u, 0u, 0u};
        if (k == 32) b = *reinterpret_cast<const u32x4*>(p + 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v.w[i] = a[i]; v.w[4 + i] = b[i]; }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v.w[i] = 0u;
#pragma unroll
        for (int i = 0; i < 32; ++i)
            if (i < k) v.w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    }
    return v;
}
template <bool VEC> __device__ __forceinline__ void pv_store(uint8_t* p, int k, const PVec& v) {
    if constexpr (VEC) {
        u32x4 a, b;
#pragma unroll
        for (int i = 0; i < 4; ++i) { a[i] = v.w[i]; b[i] = v.w[4 + i]; }
        *reinterpret_cast<u32x4*>(p) = a;
        if (k == 32) *reinterpret_cast<u32x4*>(p + 16) = b;
    } else {
#pragma unroll
        for (int i = 0; i < 32; ++i)
            if (i < k) p[i] = (uint8_t)(v.w[i >> 2] >> (8 * (i & 3)));
    }
}
// bit j: byte j of the vector is non-zero.  Per word: the top bit of every non-zero byte, then the four bits gathered by
// one multiply (the partial products land on distinct bits, so nothing carries).
__device__ __forceinline__ uint32_t pv_nonzero(const PVec& v) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t x = v.w[i];
        const uint32_t t = ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;
        m |= ((t * 0x10204080u) >> 28) << (4 * i);
    }
    return m;
}
// byte j (wave-uniform j) of the vector; selects, so the vector stays in registers
__device__ __forceinline__ uint32_t pv_get(const PVec& v, int j) {
    uint32_t x = v.w[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) x = (j >> 2) == i ? v.w[i] : x;
    return (x >> (8 * (j & 3))) & 0xffu;
}
__device__ __forceinline__ void pv_put(PVec& v, int j, uint32_t byte) {
    const uint32_t x = byte << (8 * (j & 3));
#pragma unroll
    for (int i = 0; i < 8; ++i) v.w[i] |= (j >> 2) == i ? x : 0u;
}

// ---- what a workgroup knows about its image ------------------------------------------------------------------------------
struct CpImage {
    int s;                       // the source image, -1: none
    int flip, nb, ns;
    long dy, dx;
};
__device__ __forceinline__ int cp_clamp(int v, int k) { return min(max(v, 0), k); }
__device__ __forceinline__ CpImage cp_image(const CpArgs& a, int b) {
    CpImage g;
    const int s = a.xform[4 * b];
    g.s = (s >= 0 && s < a.n) ? s : -1;
    g.flip = a.xform[4 * b + 1];
    g.dy = a.xform[4 * b + 2];
    g.dx = a.xform[4 * b + 3];
    g.nb = cp_clamp(a.n_objects[b], a.k);
    g.ns = g.s >= 0 ? cp_clamp(a.n_objects[g.s], a.k) : 0;
    return g;
}
// the source pixel of target pixel (y, x): its index in the image, -1 out of frame
__device__ __forceinline__ int cp_source(const CpImage& g, int y, int x, int h, int w) {
    const long u = x - g.dx, v = y - g.dy;
    if (u < 0 || u >= w || v < 0 || v >= h) return -1;
    const int xs = (g.flip & 1) ? w - 1 - (int)u : (int)u, ys = (g.flip & 2) ? h - 1 - (int)v : (int)v;
    return ys * w + xs;
}
// the paste set from the area counters: {pasted bits, their count, the area-limited flag}
struct CpSet { uint32_t bits; int count, flag; };
__device__ __forceinline__ CpSet cp_set(const CpArgs& a, const CpImage& g, int b) {
    CpSet p = {0u, 0, 0};
    if (g.s < 0) return p;
    const uint32_t sel = a.select[b];
    const int cap = a.k - g.nb, thr = max(a.min_area, 1);
    for (int j = 0; j < g.ns; ++j) {
        if (!((sel >> j) & 1u)) continue;
        if (a.area[(long)b * a.k + j] >= thr && p.count < cap) { p.bits |= 1u << j; ++p.count; }
        else p.flag = 1;
    }
    return p;
}

// Counting pixels per plane.  cp_count, called by every lane of a wave with its pixel's mask, adds to `mine` of lane j the
// number of lanes whose mask has bit j (j < k).  cp_flush, called once by all lanes of the workgroup after the walk, folds
// the waves in LDS and adds one atomic per plane to dst[0..k).
__device__ __forceinline__ void cp_count(uint32_t mask, int k, int lane, uint32_t& mine) {
    if (__ballot(mask != 0u) == 0ull) return;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (j < k) {
            const uint32_t cnt = (uint32_t)__popcll(__ballot((mask >> j) & 1u));
            mine += lane == j ? cnt : 0u;
        }
    }
}
__device__ __forceinline__ void cp_flush(uint32_t mine, int k, uint32_t* sh, int32_t* dst) {
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 32) sh[threadIdx.x] = 0u;
    __syncthreads();
    if (lane < k && mine != 0u) atomicAdd(&sh[lane], mine);
    __syncthreads();
    if ((int)threadIdx.x < k && sh[threadIdx.x] != 0u) atomicAdd(dst + threadIdx.x, (int32_t)sh[threadIdx.x]);
}

// ---- launch 0: the counters start at zero (a kernel, not a memset node: the sequence is kernels alone under capture) ---------
__global__ __launch_bounds__(CP_THREADS) void cp_clear_kernel(int32_t* counters, long count) {
    for (long i = (long)blockIdx.x * CP_THREADS + threadIdx.x; i < count; i += (long)gridDim.x * CP_THREADS) counters[i] = 0;
}

// ---- launch 1: the areas ------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(CP_THREADS) void cp_areas_kernel(CpArgs a) {
    __shared__ uint32_t sh[32];
    const int b = blockIdx.y;
    const CpImage g = cp_image(a, b);
    if (g.s < 0 || g.ns == 0) return;
    // the in-frame window of the target: x in [x0, x1), y in [y0, y1)
    const long x0 = max(0L, g.dx), x1 = min((long)a.w, a.w + g.dx), y0 = max(0L, g.dy), y1 = min((long)a.h, a.h + g.dy);
    if (x1 <= x0 || y1 <= y0) return;
    const int ww = (int)(x1 - x0), total = ww * (int)(y1 - y0), lane = threadIdx.x & 63;
    const uint8_t* src = a.planes + (long)g.s * a.h * a.w * a.k;
    const uint32_t real = g.ns >= 32 ? 0xffffffffu : (1u << g.ns) - 1u;
    uint32_t mine = 0;
    for (int base = blockIdx.x * CP_THREADS; base < total; base += gridDim.x * CP_THREADS) {
        const int q = base + threadIdx.x;
        uint32_t m = 0;
        if (q < total) {
            const int sp = cp_source(g, (int)y0 + q / ww, (int)x0 + q % ww, a.h, a.w);
            if (sp >= 0) m = pv_nonzero(pv_load<VEC>(src + (long)sp * a.k, a.k)) & real;
        }
        cp_count(m, a.k, lane, mine);
    }
    cp_flush(mine, a.k, sh, a.area + (long)b * a.k);
}

// ---- launch 2: apply ----------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(CP_THREADS) void cp_apply_kernel(CpArgs a) {
    __shared__ uint32_t sh[32];
    __shared__ uint32_t set_bits;
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const CpImage g = cp_image(a, b);
    if (threadIdx.x == 0) set_bits = cp_set(a, g, b).bits;
    __syncthreads();
    const uint32_t pbits = set_bits;
    const int hw = a.h * a.w, k = a.k, c = a.c;
    const long img = (long)b * hw, simg = (long)max(g.s, 0) * hw;
    uint32_t keep[8];                                    // the bytes of the target planes [0, n_b)
#pragma unroll
    for (int i = 0; i < 8; ++i) keep[i] = g.nb >= 4 * i + 4 ? 0xffffffffu : g.nb <= 4 * i ? 0u : (1u << (8 * (g.nb - 4 * i))) - 1u;
    uint32_t mine = 0;
    for (int base = blockIdx.x * CP_THREADS; base < hw; base += gridDim.x * CP_THREADS) {
        const int q = base + threadIdx.x;
        uint32_t left = 0;
        if (q < hw) {
            PVec t = pv_load<VEC>(a.planes + (img + q) * k, k);
#pragma unroll
            for (int i = 0; i < 8; ++i) t.w[i] &= keep[i];
            long from = img + q;                         // where rgb and sem come from
            if (pbits != 0u) {
                const int sp = cp_source(g, q / a.w, q % a.w, a.h, a.w);
                if (sp >= 0) {
                    const PVec s = pv_load<VEC>(a.planes + (simg + sp) * k, k);
                    if (pv_nonzero(s) & pbits) {         // M: the pixel is covered; its target planes go, the pasted ones come
                        from = simg + sp;
#pragma unroll
                        for (int i = 0; i < 8; ++i) t.w[i] = 0u;
                        int slot = g.nb;
                        for (uint32_t rest = pbits; rest != 0u; rest &= rest - 1u, ++slot) pv_put(t, slot, pv_get(s, __ffs(rest) - 1));
                    }
                }
                left = pv_nonzero(t) & (g.nb >= 32 ? 0xffffffffu : (1u << g.nb) - 1u);   // the pasted slots lie at or above n_b
            }
            pv_store<VEC>(a.planes_out + (img + q) * k, k, t);
            a.sem_out[img + q] = a.sem[from];
            for (int ch = 0; ch < c; ++ch) a.rgb_out[(img + q) * c + ch] = a.rgb[from * c + ch];
        }
        if (pbits != 0u) cp_count(left, k, lane, mine);
    }
    if (pbits != 0u) cp_flush(mine, k, sh, a.remain + (long)b * k);
}

// ---- launch 3: compact --------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(CP_THREADS) void cp_compact_kernel(CpArgs a) {
    __shared__ int map[32];                              // output plane o takes plane map[o] of what launch 2 wrote
    __shared__ int n_out_sh, moved_sh;
    const int b = blockIdx.y, k = a.k;
    if (threadIdx.x == 0) {
        const CpImage g = cp_image(a, b);
        const CpSet p = cp_set(a, g, b);
        uint32_t kept = 0;
        int o = 0;
        for (int i = 0; i < g.nb; ++i)
            if (p.bits == 0u || a.remain[(long)b * k + i] > 0) { kept |= 1u << i; map[o++] = i; }
        const int moved = o != g.nb;
        for (int r = 0; r < p.count; ++r) map[o++] = g.nb + r;
        n_out_sh = o;
        moved_sh = moved;
        if (blockIdx.x == 0) {
            a.n_out[b] = o;
            a.plan[4 * b] = (int32_t)p.bits;
            a.plan[4 * b + 1] = (int32_t)kept;
            a.plan[4 * b + 2] = o;
            a.plan[4 * b + 3] = p.flag;
        }
    }
    __syncthreads();
    if (!moved_sh) return;
    const int n_out = n_out_sh, hw = a.h * a.w;
    uint8_t* img = a.planes_out + (long)b * hw * k;
    for (int q = blockIdx.x * CP_THREADS + threadIdx.x; q < hw; q += gridDim.x * CP_THREADS) {
        const PVec v = pv_load<VEC>(img + (long)q * k, k);
        if (pv_nonzero(v) == 0u) continue;               // a dropped plane holds no byte: an all-zero vector stays as it is
        PVec t;
#pragma unroll
        for (int i = 0; i < 8; ++i) t.w[i] = 0u;
        for (int o = 0; o < n_out; ++o) pv_put(t, o, pv_get(v, map[o]));
        pv_store<VEC>(img + (long)q * k, k, t);
    }
}


template <bool VEC> void cp_launch(const CpArgs& a, hipStream_t st) {
    const long hw = (long)a.h * a.w;
    const int chunks = (int)min((long)CP_MAX_CHUNKS, max(1L, (hw + CP_THREADS * CP_PIX_PER_LANE - 1) / (CP_THREADS * CP_PIX_PER_LANE)));
    const dim3 grid(chunks, a.n), block(CP_THREADS);
    const long counters = 2L * a.n * a.k;
    hipLaunchKernelGGL(cp_clear_kernel, dim3(grid_cap((counters + CP_THREADS - 1) / CP_THREADS)), block, 0, st, a.area, counters);
    hipLaunchKernelGGL(cp_areas_kernel<VEC>, grid, block, 0, st, a);
    hipLaunchKernelGGL(cp_apply_kernel<VEC>, grid, block, 0, st, a);
    hipLaunchKernelGGL(cp_compact_kernel<VEC>, grid, block, 0, st, a);
}

}  // namespace

extern "C" int isa_copy_paste_u8(const uint8_t* rgb, const uint8_t* sem, const uint8_t* planes, const int32_t* n_objects,
                                 const int32_t* xform, const uint32_t* select, int32_t n, int32_t h, int32_t w, int32_t c,
                                 int32_t k, int32_t min_area, uint8_t* rgb_out, uint8_t* sem_out, uint8_t* planes_out,
                                 int32_t* n_out, int32_t* plan, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!rgb || !sem || !planes || !n_objects || !xform || !select || !rgb_out || !sem_out || !planes_out || !n_out || !plan ||
        !scratch)
        return ISA_EINVAL;
    if (n < 1 || n > 65535 || h < 1 || h > ISA_PASTE_MAX_SIDE || w < 1 || w > ISA_PASTE_MAX_SIDE || c < 1 || c > 4 || k < 1 ||
        k > ISA_PASTE_MAX_PLANES)
        return ISA_EINVAL;
    const uintptr_t px = (uintptr_t)n * h * w, counters = (uintptr_t)ISA_COPY_PASTE_SCRATCH_BYTES(n, k);
    // an output over any input (another target may still read image b as its source), or over another output or the scratch
    const struct { const void* p; uintptr_t bytes; } in[] = {{rgb, px * c}, {sem, px}, {planes, px * k}, {n_objects, (uintptr_t)n * 4},
                                                              {xform, (uintptr_t)n * 16}, {select, (uintptr_t)n * 4}},
                                                     out[] = {{rgb_out, px * c}, {sem_out, px}, {planes_out, px * k},
                                                              {n_out, (uintptr_t)n * 4}, {plan, (uintptr_t)n * 16}, {scratch, counters}};
    for (const auto& o : out)
        for (const auto& i : in)
            if (ranges_overlap(o.p, o.bytes, i.p, i.bytes)) return ISA_EINVAL;
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            if (ranges_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes)) return ISA_EINVAL;
    const bool vec = k % 16 == 0;
    if (!aligned(n_objects, 4) || !aligned(xform, 4) || !aligned(select, 4) || !aligned(n_out, 4) || !aligned(plan, 4) ||
        !aligned(scratch, 4) || (vec && (!aligned(planes, 16) || !aligned(planes_out, 16))))
        return ISA_EALIGN;
    if (scratch_bytes < ISA_COPY_PASTE_SCRATCH_BYTES(n, k)) return ISA_ENOMEM;
    hipStream_t st = as_stream(stream);
    CpArgs a;
    a.rgb = rgb; a.sem = sem; a.planes = planes; a.n_objects = n_objects; a.xform = xform; a.select = select;
    a.n = n; a.h = h; a.w = w; a.c = c; a.k = k; a.min_area = min_area;
    a.rgb_out = rgb_out; a.sem_out = sem_out; a.planes_out = planes_out; a.n_out = n_out; a.plan = plan;
    a.area = reinterpret_cast<int32_t*>(scratch);
    a.remain = a.area + (long)n * k;
    if (vec) cp_launch<true>(a, st);
    else cp_launch<false>(a, st);
    return launch_status();
}
