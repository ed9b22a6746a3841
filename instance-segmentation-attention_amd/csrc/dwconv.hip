// Depthwise 3x3 (pad 1, stride 1) on NHWC: forward, data gradient, weight gradient, and the fused BatchNorm backward
// around it.  Replaces nn.Conv2d(groups=C) in InvertedV1Residual / InvertedResidual / the instance stems.  No MFMA: a
// 9-tap per-channel stencil.  Every kernel here works on LDS-staged halo tiles of whole 8-channel vectors, so a view
// qualifies when its row pitch covers rup(C, 8) (tensor_ok(., 8) guarantees it: the 21-channel input lives in 24-channel
// rows; pad lanes compute values that no consumer reads and no statistic sees).
//   * a workgroup owns an 8 x 32 output tile x 32 channels.  The (8+2) x (32+2) input halo is staged ONCE
//     in LDS as fp32 after the lazy BN/ReLU6 prologue: every lane issues its 5-6 independent 16-byte
//     loads back to back, so ~24 KB per workgroup is in flight (a register-window walk over row strips, with 3
//     dependent loads per column, was latency-bound: 62 % SQ_WAIT_ANY at 2 waves/SIMD).
//   * compute: lane = (8-channel group, 4 consecutive x): 18 row vectors from LDS feed 36 FMA-vectors for
//     4 outputs (horizontal register reuse), pixel stride padded to 36 floats so the four x-groups of a
//     16-lane ds_read_b128 group land on disjoint banks.
//   * forward/dgrad: bias, next-BN statistics (16-lane shuffle tree, then 4 LDS atomics per wave, then one
//     global atomic per channel into the replicated buffer), optional read-modify-write accumulate.
//   * wgrad: persistent over tiles of one channel block; 9x8 products per lane accumulated in registers
//     across tiles, reduced once (shuffle tree + LDS) into a per-workgroup slab (no global atomics).
#include "common.hpp"
#include <type_traits>

namespace {

constexpr int TH = 8, TW = 32, CB = 32, PS = 36;         // tile rows/cols, channel block, pixel stride (floats)
constexpr int HALO = (TH + 2) * (TW + 2);

struct Dw2Params {
    const void* x; const void* w; const float* bias; void* y; const void* dy;
    int n, h, w_, c, ldx, ldy, ldd, wld;
    ProDev pro;
    float* stats; int accumulate;
    int tiles_x, tiles_y; long ntiles;
    float* ws; int csrc;
    int G;                       // statistic groups: n and ntiles are per group (common.hpp)
    FinDev fin;                  // pending BatchNorm finalize of the lazy input (forward only), or stats == NULL
};

// raw8<T> (common.hpp): 8 storage elements kept packed in registers until they are consumed

// per-lane prologue constants: a lane stages the same 8-channel group on every iteration (i += 256 keeps i & 3)
struct ProRegs { float sc[8], sh[8], bs[8]; };

template <bool HAS_PRO>
__device__ __forceinline__ void load_pro(const Dw2Params& p, ProRegs& r, int c0, int b) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = min(c0 + j, p.c - 1);
        r.sc[j] = (HAS_PRO && p.pro.scale) ? p.pro.scale[c] : 1.f;
        r.sh[j] = (HAS_PRO && p.pro.shift) ? p.pro.shift[c] : 0.f;
        r.bs[j] = (HAS_PRO && p.pro.bscale) ? p.pro.bscale[(long)b * p.c + c] : 1.f;
    }
}

template <typename T, bool HAS_PRO, int ACT>
__device__ __forceinline__ void stage_tile(const Dw2Params& p, const ProRegs& r, float* tile, int b, int ty, int tx, int c_base) {
    const T* xin = reinterpret_cast<const T*>(p.x);
    const int cg = threadIdx.x & 3;
    const int c0 = c_base + cg * 8;
    const bool cok = c0 < p.c;
    constexpr int NIT = (HALO * 4 + 255) / 256;
    float v[NIT][8];
    bool ok[NIT];
    // all global loads first (independent, in flight together), then prologue + LDS stores
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int pix = (threadIdx.x + it * 256) >> 2;
        const int rr = pix / (TW + 2), cc = pix - rr * (TW + 2);
        const int gy = ty * TH + rr - 1, gx = tx * TW + cc - 1;
        ok[it] = pix < HALO && cok && gy >= 0 && gy < p.h && gx >= 0 && gx < p.w_;
        if (ok[it]) load8<T>(xin + (((long)b * p.h + gy) * p.w_ + gx) * p.ldx + c0, v[it]);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int pix = (threadIdx.x + it * 256) >> 2;
        if (pix >= HALO) continue;
        f32x4 a, bb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float z = 0.f;
            if (ok[it]) {
                z = v[it][j];
                if constexpr (HAS_PRO) {
                    z = act_t<ACT>(fmaf(z, r.sc[j], r.sh[j]), p.pro.act);
                    if (p.pro.bscale) z *= r.bs[j];
                }
            }
            if (j < 4) a[j] = z; else bb[j - 4] = z;
        }
        *reinterpret_cast<f32x4*>(tile + pix * PS + cg * 8) = a;
        *reinterpret_cast<f32x4*>(tile + pix * PS + cg * 8 + 4) = bb;
    }
}

// acc[j] += x[j] * w[j] for 8 channels as four v_pk_fma_f32 (packed fp32: two FMAs per lane per issue)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void fma8(const float (&x)[8], const float (&w)[8], float (&acc)[8]) {
#ifdef ISA_DW_SCALAR_FMA
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(x[j], w[j], acc[j]);
#else
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const f32x2 r = __builtin_elementwise_fma(f32x2{x[j], x[j + 1]}, f32x2{w[j], w[j + 1]}, f32x2{acc[j], acc[j + 1]});
        acc[j] = r[0]; acc[j + 1] = r[1];
    }
#endif
}

__device__ __forceinline__ void ld8(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
}

// XCD-aware tile walk for the persistent kernels: workgroup b runs on XCD b % 8 (round-robin dispatch), each XCD has its
// own L2.  Adjacent tiles share halo rows / columns, so each XCD gets ONE contiguous eighth of the tile sequence and
// its workgroups stride inside it: the halo overlap is re-read from that XCD's L2 instead of from seven other ones.
struct TileRange { long t0, end, step; };
// (bx, nbx): the workgroup's index and the workgroup count inside its statistic group (GroupSel); with nbx % 8 == 0 a
// group starts on XCD 0, so bx & 7 is still the XCD
__device__ __forceinline__ TileRange tile_range(long ntiles, int bx, int nbx) {
    if ((nbx & 7) == 0 && ntiles >= 64) {
        const int xcd = bx & 7, j = bx >> 3;
        const long chunk = (ntiles + 7) / 8;
        const long end = min(ntiles, (xcd + 1) * chunk);
        return TileRange{xcd * chunk + j, end, (long)(nbx >> 3)};
    }
    return TileRange{(long)bx, ntiles, (long)nbx};
}

// Tile coordinates kept incrementally: the tile sequence of a workgroup is t0, t0 + step, ... and a 64-bit
// `t % tiles_x`, `t / tiles_x % tiles_y` pair per tile per role cost more scalar instructions than the tile's loads
// (ablation: with every load, LDS access, FMA and store removed the forward kernel still took 39 of its 93 us - the
// per-tile bookkeeping; one wave per role and SIMD issues an instruction every >= 4 cycles).  All fields are
// wave-uniform (SGPRs).
struct TileIter {
    long t, end, step;
    int tx, ty, b, sx, sy, sb, ntx, nty;
    __device__ __forceinline__ void init(const TileRange& r, int tiles_x, int tiles_y) {
        t = r.t0; end = r.end; step = r.step; ntx = tiles_x; nty = tiles_y;
        long q = t / tiles_x; tx = (int)(t - q * tiles_x); b = (int)(q / tiles_y); ty = (int)(q - (long)b * tiles_y);
        long qs = step / tiles_x; sx = (int)(step - qs * tiles_x); sb = (int)(qs / tiles_y); sy = (int)(qs - (long)sb * tiles_y);
    }
    __device__ __forceinline__ bool valid() const { return t < end; }
    __device__ __forceinline__ void next() {
        t += step;
        tx += sx; const int c = tx >= ntx ? 1 : 0; tx -= c * ntx;
        ty += sy + c; const int c2 = ty >= nty ? 1 : 0; ty -= c2 * nty;
        b += sb + c2;
    }
};

// Tiles the double-buffered loader keeps in flight ahead of the one it converts (12 VGPRs per tile in bf16).  Measured
// on HBM-cold operands: two tiles ahead is 0-7 % slower than one at every shape of the training step
#ifndef ISA_DW_FWD_PF
#define ISA_DW_FWD_PF 1
#endif

// Persistent over tiles of one channel block.  DB (bf16): 768 threads, waves 4-11 stage the next tile into the other
// LDS buffer while waves 0-3 run the stencil on the current one (the same role split as dw_bn_bwd_kernel below);
// weights, prologue constants and the statistic partial sums live across tiles and are flushed once.
//  * The loader is software-pipelined across tiles like the fused backward's: the halo loads are UNCONDITIONAL at a
//    clamped address (zeroed by selects at conversion), so the tile loop is straight-line code, the loads of the next
//    ISA_DW_FWD_PF tiles are in flight while a tile is converted and while the loader waits at the barrier, and every
//    vmcnt wait is partial.  With one predicated load per exec-mask region the compiler waited vmcnt(0) per tile and a CU
//    had at most one halo tile (21.8 KB) outstanding, none during conversion: ~1.6 TB/s of reads by Little's law.
//  * ACC: the data-gradient entry point may accumulate into the old output.  Only a launch that does takes the variant
//    with the operand; every other one compiles it out: its compute role issues no global load, so it has no vmcnt wait
//    in the tile loop (vmcnt also counts stores: the run-time flag made every tile wait for the previous tile's output
//    stores, inside the stencil or - with the loads hoisted - ahead of each store).
//  * Launch prologue: the loader's first tiles are the kernel's first memory instructions; weights, bias and the
//    prologue constants are requested behind them through pointer selects (a null optional pointer reads element 0 of x,
//    which always exists, and the value is replaced by the neutral constant) - one round trip and one wait ahead of the
//    single barrier instead of ~ten dependent ones.  A pending finalize keeps its own dependency (and barrier).
// Clamped addresses stay inside the tensor: an in-image slot reads channels [c0, c0 + 8) of an image pixel with
// c0 < c, c0 % 8 == 0, so c0 + 8 <= rup(c, 8) <= ld (tensor_ok(., 8)); every other slot (outside the image, past
// HALO, or a channel group with c0 >= c) reads the tile's origin pixel (b, ty * TH, tx * TW), which is inside the image
// for every tile of the walk, at channel offset c0 if c0 < c, else c_base: c_base = 32 * blockIdx.y < c because
// gridDim.y = ceil(c / 32), and c_base + 8 <= rup(c, 8) <= ld again.  Both hold for c % 32 != 0 and for ld > c.
template <typename T, bool HAS_PRO, int ACT, bool DB, bool ACC>
__global__ __launch_bounds__(DB ? 768 : 256) __attribute__((amdgpu_waves_per_eu(2, 3))) void dw2_fwd_kernel(Dw2Params p) {
    // DB: waves 0-3 compute, waves 4-11 stage (three waves per SIMD: the staging arithmetic of a tile is spread over
    // twice the lanes and the SIMD has one more wave to issue from while the others wait)
    constexpr int NTHR = DB ? 768 : 256;
    constexpr int LTHR = DB ? 512 : 256;              // threads that stage a tile
    constexpr int NBUF = DB ? 2 : 1;
    constexpr int PF = ISA_DW_FWD_PF;
    static_assert(PF == 1 || PF == 2, "prefetch distance in tiles");
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* tile_base = sm;                          // [NBUF][HALO][PS]
    float* wts = sm + NBUF * HALO * PS;             // [9][CB]
    float* red = wts + 9 * CB;                      // [2*CB]
    float* fin_tab = red + 2 * CB;                  // [2][CB] scale / shift of this channel block when the finalize runs here
    const int tid = threadIdx.x;
    const bool loader = DB && tid >= 256;
    const bool stager = !DB || loader;                // this lane stages tiles
    const int ltid = loader ? tid - 256 : tid;        // index inside the role group
    const int c_base = blockIdx.y * CB;
    const GroupSel gs = group_sel(p.G);
    if (gs.g) {                                       // this workgroup's statistic group: its n images, its constants
        const long img = (long)gs.g * p.n, pix = img * p.h * p.w_;
        p.x = reinterpret_cast<const T*>(p.x) + pix * p.ldx;
        p.y = reinterpret_cast<T*>(p.y) + pix * p.ldy;
        p.pro.scale = goff(p.pro.scale, (long)gs.g * p.c); p.pro.shift = goff(p.pro.shift, (long)gs.g * p.c);
        p.pro.bscale = goff(p.pro.bscale, img * p.c);
        p.stats = goff(p.stats, (long)gs.g * ISA_STAT_R * 2 * p.c);
    }
    const T* wp = reinterpret_cast<const T*>(p.w);
    const int cg = ltid & 3, g = ltid >> 2, row = g >> 3, x0 = (g & 7) * 4;
    const int c0 = c_base + cg * 8;
    const bool cok = c0 < p.c;
    const int cc0 = cok ? c0 : c_base;
    const T* xin = reinterpret_cast<const T*>(p.x);
    constexpr int NIT = (HALO * 4 + LTHR - 1) / LTHR;
    const bool has_bs = HAS_PRO && p.pro.bscale;             // wave-uniform

    // tile-invariant part of the staging addresses: halo pixel (rr, cc) of slot `it` and its element offset from the
    // tile's halo origin; per tile only a scalar base pointer and (on border tiles) four scalar bounds remain
    int hrc[NIT], hoff[NIT];
    bool hok[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int pix = (ltid + it * LTHR) >> 2;
        const int rr = pix / (TW + 2), cc = pix - rr * (TW + 2);
        hrc[it] = (rr << 16) | cc;
        hoff[it] = (rr * p.w_ + cc) * p.ldx + cc0;
        hok[it] = pix < HALO && cok;
    }
    const int soff = (p.w_ + 1) * p.ldx + cc0;                 // halo (1, 1) = the tile's origin pixel: the clamp target
    const int ooff = (row * p.w_ + x0) * p.ldy + c0;           // output element offset from the tile's origin

    struct Geo { const T* base; int b, rlo, rhi, clo, chi; bool interior; };
    auto geo = [&](int b, int ty, int tx) {
        Geo q;
        q.base = xin + (((long)b * p.h + ty * TH - 1) * p.w_ + tx * TW - 1) * p.ldx;   // halo origin (may lie outside)
        q.b = b;
        // scalar bounds of the in-image part of the halo, in halo coordinates
        q.rlo = 1 - ty * TH; q.rhi = p.h + 1 - ty * TH; q.clo = 1 - tx * TW; q.chi = p.w_ + 1 - tx * TW;
        q.interior = q.rlo <= 0 && q.rhi >= TH + 2 && q.clo <= 0 && q.chi >= TW + 2;
        return q;
    };
    auto slot_ok = [&](const Geo& q, int it) {
        const int rr = hrc[it] >> 16, cc = hrc[it] & 0xffff;
        return hok[it] && (q.interior || (rr >= q.rlo && rr < q.rhi && cc >= q.clo && cc < q.chi));
    };
    // The empty asm keeps a load where it is written (see dw_bn_bwd_kernel::issue): LLVM otherwise sinks a prefetch to
    // its first use, across the LDS-only barrier and the loop back-edge.
    auto issue = [&](const Geo& q, int it, raw8<T>& v) {
        v.load(q.base + (slot_ok(q, it) ? hoff[it] : soff));
        asm volatile("" ::: "memory");
    };

    // ---- launch prologue: everything but the tile loads, requested in one round trip.  Each role calls it once (the
    // loader behind its first tiles' loads, so the tile registers live on the loader side only); b_first: image of the
    // loader's first tile.  Ends with the barrier that publishes the weights and the zeroed `red`.
    float bv[8], sc[8], sh[8], bs[8];
    auto prologue = [&](int b_first) {
    const float* dummy = reinterpret_cast<const float*>(p.x);   // always present, 16-byte aligned, >= 16 bytes
    constexpr int NW = (9 * CB + NTHR - 1) / NTHR;
    float wv[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int i = min(tid + k * NTHR, 9 * CB - 1);
        const int tp = i / CB, cc = i - tp * CB;
        wv[k] = st<T>::ld(wp + (long)tp * p.wld + min(c_base + cc, p.c - 1));
    }
    // a pending finalize of the input's BatchNorm produces scale / shift below: the arrays are not read here then
    const bool fin_pending = HAS_PRO && p.fin.stats != nullptr;
    const bool ld_sc = HAS_PRO && p.pro.scale && !fin_pending, ld_sh = HAS_PRO && p.pro.shift && !fin_pending;
    if (!loader) {                                              // the compute role's bias, kept in registers across tiles
        const float* bp = p.bias ? p.bias : dummy;
#pragma unroll
        for (int j = 0; j < 8; ++j) bv[j] = bp[p.bias ? min(c0 + j, p.c - 1) : 0];
    }
    if (HAS_PRO && stager) {
        const float* sp = ld_sc ? p.pro.scale : dummy;
        const float* hp = ld_sh ? p.pro.shift : dummy;
        const float* mp = (DB && has_bs) ? p.pro.bscale + (long)b_first * p.c : dummy;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = min(c0 + j, p.c - 1);
            sc[j] = sp[ld_sc ? c : 0];
            sh[j] = hp[ld_sh ? c : 0];
            if constexpr (DB) bs[j] = mp[has_bs ? c : 0];
        }
    }
    asm volatile("" ::: "memory");
    // a pending finalize of the input's BatchNorm runs here, for this workgroup's 32 channels, behind the requests
    // above; the last workgroup of each channel block writes the arrays the backward pass reads
    const bool fin = HAS_PRO && bn_fin_inline<NTHR>(p.fin, p.c, p.G, gs.g, fin_tab, CB, tid, c_base, CB,
                                                    blockIdx.x == gridDim.x - 1 && blockIdx.z == 0);
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int i = tid + k * NTHR;
        if (i < 9 * CB) wts[i] = (c_base + (i & (CB - 1)) < p.c) ? wv[k] : 0.f;
    }
    if (tid < 2 * CB) red[tid] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = min(c0 + j, p.c - 1);
        bv[j] = (p.bias && c0 + j < p.c) ? bv[j] : 0.f;
        sc[j] = ld_sc ? sc[j] : 1.f;
        sh[j] = ld_sh ? sh[j] : 0.f;
        if (fin) { sc[j] = fin_tab[c - c_base]; sh[j] = fin_tab[CB + c - c_base]; }
        bs[j] = (DB && has_bs) ? bs[j] : 1.f;                    // z * 1.f == z bit for bit: no branch in convert
    }
    __syncthreads();                                             // weights + zeroed `red` visible
    };

    // one halo slot: lazy prologue, zero outside the image, fp32 into the LDS tile
    auto convert = [&](bool ok, int it, const raw8<T>& r, float* tile) {
        const int pix = (ltid + it * LTHR) >> 2;
        if (pix >= HALO) return;
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float z = r.get(j);
            if constexpr (HAS_PRO) z = act_t<ACT>(fmaf(z, sc[j], sh[j]), p.pro.act);
            o[j] = z;
        }
        if constexpr (HAS_PRO) {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] *= bs[j];
        }
        // slots outside the image were fetched from the tile's origin pixel: zero them.  Interior tiles have none
        // (uniform over the wave), so the selects are skipped there
        if (__builtin_amdgcn_ballot_w64(!ok) != 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = ok ? o[j] : 0.f;
        }
        store8<float>(tile + pix * PS + cg * 8, o);
    };

    // single-buffer form: one tile, all loads then all conversions; the per-image scale row is refetched only when the
    // image changes
    int bs_img = -1;
    auto stage = [&](int b, int ty, int tx, float* tile) {
        if (has_bs && b != bs_img) {
#pragma unroll
            for (int j = 0; j < 8; ++j) bs[j] = p.pro.bscale[(long)b * p.c + min(c0 + j, p.c - 1)];
            bs_img = b;
        }
        const Geo q = geo(b, ty, tx);
        raw8<T> r[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) issue(q, it, r[it]);
#pragma unroll
        for (int it = 0; it < NIT; ++it) convert(slot_ok(q, it), it, r[it], tile);
    };

    auto compute = [&](int b, int ty, int tx, const float* tile, float (&s1)[8], float (&s2)[8]) {
        T* ybase = reinterpret_cast<T*>(p.y) + (((long)b * p.h + ty * TH) * p.w_ + tx * TW) * p.ldy;   // tile origin
        const bool rowok = ty * TH + row < p.h && cok;
        const int xlim = p.w_ - tx * TW;                          // x0 + o < xlim
        // the old output (data gradient only): requested before the stencil at a clamped address, used after it
        raw8<T> oc[4];
        if constexpr (ACC) {
#pragma unroll
            for (int o = 0; o < 4; ++o) oc[o].load(ybase + ((rowok && x0 + o < xlim) ? ooff + o * p.ldy : cc0));
            asm volatile("" ::: "memory");
        }
        float acc[4][8];
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[o][j] = bv[j];
#pragma unroll 1
        for (int dy = 0; dy < 3; ++dy) {
            float wr[3][8], in[6][8];
#pragma unroll
            for (int k = 0; k < 3; ++k) ld8(wts + (dy * 3 + k) * CB + cg * 8, wr[k]);
#pragma unroll
            for (int k = 0; k < 6; ++k) ld8(tile + ((row + dy) * (TW + 2) + x0 + k) * PS + cg * 8, in[k]);
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    fma8(in[o + k], wr[k], acc[o]);
        }
        if (rowok) {
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (x0 + o >= xlim) continue;
                T* dst = ybase + ooff + o * p.ldy;
#pragma unroll
                for (int j = 0; j < 8; ++j) { s1[j] += acc[o][j]; s2[j] += acc[o][j] * acc[o][j]; }
                if constexpr (ACC) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[o][j] += oc[o].get(j);
                }
                store8<T>(dst, acc[o]);
            }
        }
    };

    if (loader) {
        // Barriers: one per staged tile (the first is the compute side's "first tile staged", every later one closes the
        // compute side's previous tile) plus one closing its last tile: n + 1 on both sides.  Slot d of the register
        // ring holds tiles d, d + PF, ...; a slot is refilled, load by load, right after its conversion consumed it.
        if constexpr (DB) {
            TileIter tn;                                         // the next tile to request
            Geo gq[PF];
            bool val[PF];
            raw8<T> v[PF][NIT];
            tn.init(tile_range(p.ntiles, gs.bx, gs.nbx), p.tiles_x, p.tiles_y);
            // every slot is requested, a slot without a tile from tile (0, 0, 0), which always exists: the number of
            // loads in flight at the top of the steady loop is then known at compile time and its waits are partial
#pragma unroll
            for (int d = 0; d < PF; ++d) {
                val[d] = tn.valid();
                gq[d] = val[d] ? geo(tn.b, tn.ty, tn.tx) : geo(0, 0, 0);
#pragma unroll
                for (int it = 0; it < NIT; ++it) issue(gq[d], it, v[d][it]);
                tn.next();
            }
            prologue(gq[0].b);
            // per-image scale row: `bs` is the row of the tile being converted; the row of the next tile's image is
            // requested one tile ahead (into bsn) only when the image changes
            float bsn[8];
            bool bs_new = false;
            TileIter tb;
            if (has_bs) { tb.init(tile_range(p.ntiles, gs.bx, gs.nbx), p.tiles_x, p.tiles_y); tb.next(); }
            int buf = 0;
            // one tile: convert slot d into the free LDS buffer and (REFILL) request the tile PF after it into the slot
            auto step = [&](auto dsel, auto refill) {
                constexpr int d = decltype(dsel)::value;
                constexpr bool REFILL = decltype(refill)::value;
                float* tile = tile_base + buf * HALO * PS;
                const Geo gc = gq[d];
                if (has_bs) {
                    if (bs_new) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) bs[j] = bsn[j];
                    }
                    bs_new = tb.valid() && tb.b != gc.b;
                    if (bs_new) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) bsn[j] = p.pro.bscale[(long)tb.b * p.c + min(c0 + j, p.c - 1)];
                        asm volatile("" ::: "memory");
                    }
                    tb.next();
                }
                if constexpr (REFILL) {
                    gq[d] = geo(tn.b, tn.ty, tn.tx);
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        convert(slot_ok(gc, it), it, v[d][it], tile);
                        issue(gq[d], it, v[d][it]);
                    }
                    tn.next();
                } else {
#pragma unroll
                    for (int it = 0; it < NIT; ++it) convert(slot_ok(gc, it), it, v[d][it], tile);
                    val[d] = false;
                }
                lds_barrier();
                buf ^= 1;
            };
            // steady state: every slot holds a tile and PF more remain to be requested - straight-line code with the
            // same PF * NIT loads in flight at its top and bottom
            while (tn.t + (PF - 1) * tn.step < tn.end) {
                step(std::integral_constant<int, 0>{}, std::true_type{});
                if constexpr (PF > 1) step(std::integral_constant<int, 1>{}, std::true_type{});
            }
            // drain: the last tiles, fewer than PF left to request
            while (val[0]) {
                if (PF > 1 && tn.valid()) step(std::integral_constant<int, 0>{}, std::true_type{});
                else step(std::integral_constant<int, 0>{}, std::false_type{});
                if constexpr (PF > 1) {
                    if (val[1]) {
                        if (tn.valid()) step(std::integral_constant<int, 1>{}, std::true_type{});
                        else step(std::integral_constant<int, 1>{}, std::false_type{});
                    }
                }
            }
            lds_barrier();
        }
    } else {
        prologue(0);
        float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (DB) {
            TileIter ti; ti.init(tile_range(p.ntiles, gs.bx, gs.nbx), p.tiles_x, p.tiles_y);
            int buf = 0;
            lds_barrier();                                       // first tile staged
            for (; ti.valid(); ti.next()) {
                compute(ti.b, ti.ty, ti.tx, tile_base + buf * HALO * PS, s1, s2);
                lds_barrier();
                buf ^= 1;
            }
        } else {
            TileIter ti; ti.init(TileRange{(long)gs.bx, p.ntiles, (long)gs.nbx}, p.tiles_x, p.tiles_y);
            for (; ti.valid(); ti.next()) {
                stage(ti.b, ti.ty, ti.tx, tile_base);
                __syncthreads();
                compute(ti.b, ti.ty, ti.tx, tile_base, s1, s2);
                __syncthreads();
            }
        }
        if (p.stats) {
            // lanes with equal (lane & 3) share a channel group: fold the 16 of them, then 4 LDS atomics per wave
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                s1[j] = row_fold<4>(s1[j]); s2[j] = row_fold<4>(s2[j]);
            }
            if ((tid & 15) < 4) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { atomicAdd(&red[cg * 8 + j], s1[j]); atomicAdd(&red[CB + cg * 8 + j], s2[j]); }
            }
        }
    }
    __syncthreads();
    if (p.stats && tid < 2 * CB) {
        const int cc = tid & (CB - 1), which = tid / CB;
        if (c_base + cc < p.c && red[tid] != 0.f) {
            float* rep = p.stats + ((blockIdx.x + blockIdx.y) & (ISA_STAT_R - 1)) * 2 * p.c;
            atomicAdd(rep + which * p.c + c_base + cc, red[tid]);
        }
    }
}

// wgrad: slab[blockIdx.x][t*CB + cc] (t < 9) and [9*CB + cc] (bias) for channel block blockIdx.y
template <typename T, bool HAS_PRO, int ACT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void dw2_wgrad_kernel(Dw2Params p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* tile = sm;                       // [HALO][PS]
    float* red = sm + HALO * PS;            // [10*CB]
    const int tid = threadIdx.x;
    const int c_base = blockIdx.y * CB;
    const int cg = tid & 3, g = tid >> 2, row = g >> 3, x0 = (g & 7) * 4;
    const int c0 = c_base + cg * 8;
    const GroupSel gs = group_sel(p.G);
    if (gs.g) {
        const long img = (long)gs.g * p.n, pix = img * p.h * p.w_;
        p.x = reinterpret_cast<const T*>(p.x) + pix * p.ldx;
        p.dy = reinterpret_cast<const T*>(p.dy) + pix * p.ldd;
        p.pro.scale = goff(p.pro.scale, (long)gs.g * p.c); p.pro.shift = goff(p.pro.shift, (long)gs.g * p.c);
        p.pro.bscale = goff(p.pro.bscale, img * p.c);
    }
    const T* din = reinterpret_cast<const T*>(p.dy);
    float acc[9][8], db[8];
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[tp][j] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) db[j] = 0.f;
    for (long t = gs.bx; t < p.ntiles; t += gs.nbx) {
        const int tx = (int)(t % p.tiles_x); const long q = t / p.tiles_x;
        const int ty = (int)(q % p.tiles_y); const int b = (int)(q / p.tiles_y);
        ProRegs pr;
        load_pro<HAS_PRO>(p, pr, c0, b);
        __syncthreads();
        stage_tile<T, HAS_PRO, ACT>(p, pr, tile, b, ty, tx, c_base);
        // this lane's four output gradients straight from global, issued once the staging registers are free;
        // they stay in flight across the barrier
        float d[4][8];
        const int oy = ty * TH + row;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int ox = tx * TW + x0 + o;
#pragma unroll
            for (int j = 0; j < 8; ++j) d[o][j] = 0.f;
            if (oy < p.h && ox < p.w_ && c0 < p.c) load8<T>(din + (((long)b * p.h + oy) * p.w_ + ox) * p.ldd + c0, d[o]);
        }
        __syncthreads();
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int j = 0; j < 8; ++j) db[j] += d[o][j];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            float in[6][8];
#pragma unroll
            for (int k = 0; k < 6; ++k) ld8(tile + ((row + dy) * (TW + 2) + x0 + k) * PS + cg * 8, in[k]);
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    fma8(in[o + k], d[o], acc[dy * 3 + k]);
            __builtin_amdgcn_sched_barrier(0);       // keep one row of LDS reads live at a time (register budget)
        }
    }
    __syncthreads();
    for (int i = tid; i < 10 * CB; i += 256) red[i] = 0.f;
    __syncthreads();
#pragma unroll
    for (int tp = 0; tp < 10; ++tp) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = tp < 9 ? acc[tp < 9 ? tp : 0][j] : db[j];
            v = row_fold<4>(v);
            if ((tid & 15) < 4) atomicAdd(&red[tp * CB + cg * 8 + j], v);
        }
    }
    __syncthreads();
    float* slab = p.ws + ((long)blockIdx.x * gridDim.y + blockIdx.y) * 10 * CB;
    for (int i = tid; i < 10 * CB; i += 256) slab[i] = red[i];
}

// the tile grid of a launch (p.n: images per statistic group) and the workgroups in x a persistent kernel wants for it:
// `resident` over the chip, shared among the ncb channel blocks, never more than there are tiles
template <typename P> void set_tiles(P& p) {
    p.tiles_x = (p.w_ + TW - 1) / TW; p.tiles_y = (p.h + TH - 1) / TH;
    p.ntiles = (long)p.n * p.tiles_x * p.tiles_y;
}
template <typename P> long want_grid(const P& p, long resident, int ncb) {
    const long gx = resident / ncb < 1 ? 1 : resident / ncb;
    return gx > p.ntiles * p.G ? p.ntiles * p.G : gx;
}

template <typename T, bool HAS_PRO, int ACT, bool ACC = false>
int launch_fwd2_inst(Dw2Params& p, dim3 grid, hipStream_t s) {
    constexpr bool DB = sizeof(T) == 2;
    constexpr size_t lds = ((size_t)(DB ? 2 : 1) * HALO * PS + 9 * CB + 2 * CB + 2 * CB) * 4;
    static bool configured = false;
    if (!configured) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&dw2_fwd_kernel<T, HAS_PRO, ACT, DB, ACC>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return ISA_ELAUNCH;
        configured = true;
    }
    hipLaunchKernelGGL((dw2_fwd_kernel<T, HAS_PRO, ACT, DB, ACC>), grid, dim3(DB ? 768 : 256), lds, s, p);
    return launch_status();
}

// The data-gradient entry point (no prologue) is the only caller that may accumulate into the old output
template <typename T>
int launch_fwd2(Dw2Params& p, bool has_pro, hipStream_t s) {
    set_tiles(p);
    if (p.ntiles * p.G >= (1L << 31)) return ISA_EINVAL;
    const int ncb = (p.c + CB - 1) / CB;
    // persistent: bf16 = one 512-thread double-buffered workgroup per CU, f32 = three 256-thread ones
    const long gx = group_grid(want_grid(p, 256L * (sizeof(T) == 2 ? 1 : 3), ncb), p.G);
    dim3 grid((unsigned)gx, ncb);
    if (p.accumulate) return has_pro ? ISA_EINVAL : launch_fwd2_inst<T, false, ISA_ACT_NONE, true>(p, grid, s);
    if (has_pro && p.pro.act == ISA_ACT_RELU6) return launch_fwd2_inst<T, true, ISA_ACT_RELU6>(p, grid, s);
    if (has_pro) return launch_fwd2_inst<T, true, ACT_RT>(p, grid, s);
    return launch_fwd2_inst<T, false, ISA_ACT_NONE>(p, grid, s);
}

template <typename T>
int launch_wg2(Dw2Params& p, bool has_pro, long ws_floats, isa_slab_arena* sa, const isa_pro* fin, hipStream_t s) {
    set_tiles(p);
    const int ncb = (p.c + CB - 1) / CB;
    long gx;                             // 2 resident workgroups per CU
    if (int rc = slab_plan(sa, &p.ws, ws_floats, want_grid(p, 256L * 2, ncb), 10L * CB * ncb, p.G, &gx)) return rc;
    dim3 grid((unsigned)gx, ncb);
    const size_t lds = ((size_t)HALO * PS + 10 * CB) * 4;
    if (int rc = fin_standalone(fin, p.c, p.G, s)) return rc;            // every check has passed
    if (has_pro && p.pro.act == ISA_ACT_RELU6) hipLaunchKernelGGL((dw2_wgrad_kernel<T, true, ISA_ACT_RELU6>), grid, dim3(256), lds, s, p);
    else if (has_pro) hipLaunchKernelGGL((dw2_wgrad_kernel<T, true, ACT_RT>), grid, dim3(256), lds, s, p);
    else hipLaunchKernelGGL((dw2_wgrad_kernel<T, false, ISA_ACT_NONE>), grid, dim3(256), lds, s, p);
    if (launch_status() != ISA_OK) return ISA_ELAUNCH;
    return dw_slab_reduce_launch(p.ws, (float*)p.y, (float*)p.bias, (int)gx, ncb, CB, p.c, p.csrc, sa, s);
}

// ------------------------------------------------------------------------------------------------
// Fused backward of  x --dw3x3--> y --BN(train)+act--> ...   (InvertedResidual / InvertedV1Residual middle):
//   given g = dL/d act(BN(y)) and the already reduced sums of BN(y)'s backward, one pass over the tiles does
//     1. dy = gamma*invstd*(g*act'(z) - mean(g') - yhat*mean(g'*yhat))   (the BN-backward "apply", never stored)
//     2. dx (+)= dw3x3_flipped(dy)                                          (depthwise data gradient)
//     3. dW += sum  pro(x)[window] * dy                                     (depthwise weight gradient)
//     4. if x is itself a lazy BN output: the sums (sum g_x, sum g_x*xhat) its BN backward needs, from the
//        dx tile still in registers                                         (the next BN-backward "reduce")
//   replacing bn_bwd_apply (3 tensor passes) + dw_wgrad (2) + dw_dgrad (2) + bn_bwd_reduce (2) by
//   3 reads + 1 write.  dy is rounded to the storage type in LDS exactly as the unfused path rounds it in HBM.
struct FusedParams {
    const void *g, *y, *x, *w; void* dx;
    int n, h, w_, c, ldg, ldy, ldx, lddx, wld;
    const float *ysc, *ysh, *ymu, *yis, *yred; float ycnt_inv; int yact; float *ydgamma, *ydbeta;
    const float *xsc, *xsh, *xmu, *xis; int xact; float* xred;
    int accumulate, tiles_x, tiles_y; long ntiles; float* ws; int csrc; float* dw;
    const void* addend; int lda;      // optional: dx += addend (gradient of the block's residual branch)
    int G;                            // statistic groups: n and ntiles are per group (common.hpp)
};


template <typename T> struct dd_stride { static constexpr int v = 36; };       // floats: 144 B / pixel
template <> struct dd_stride<bf16_t> { static constexpr int v = 40; };         // 80 B / pixel: 4 x-groups tile 256 B

// DB (bf16): 512 threads, two LDS tile buffers.  Waves 4-7 (loader role) only stage tiles - 16-byte loads, the
// BN-backward arithmetic of dy, LDS stores - while waves 0-3 (compute role) run the two stencils on the current tile;
// one LDS-only barrier per tile swaps the buffers.  The single-buffer form (f32 storage: the tiles do not fit twice)
// runs the same phases back to back in 256 threads.
// What the measurements said (256x256x64, bf16, 223 us at the start):
//  * PMC: the single-buffer kernel waited on memory for most of each tile -> the role split.
//  * Ablation: no loads 120 us, no loader arithmetic 184 us, no stencils 201 us - every part additive.
//  * A cycle trace of one workgroup: the COMPUTE wave was the critical path.  Its epilogue loaded raw x (for the
//    BN(x) sums) from global memory, and those few loads queued in the CU's in-order vector-memory pipeline behind the
//    loader's bulk stream: every tile waited most of a tile's HBM time for them, the loader idled at the barrier.
//  -> the LDS tile now holds RAW x (storage type).  The compute role applies the lazy prologue itself (the unfused
//     arithmetic, bit for bit), takes the centre pixels for the BN(x) sums from the same tile and, in the common case,
//     reads no global memory at all.  LDS drops from 152 to 109 KB and the weight-gradient window reads halve.
//  -> the loader is software-pipelined across tiles (a tile's worth of loads always in flight) and keeps its
//     per-channel constants in registers: it is VALU-issue bound next to the compute wave of the same SIMD.
// EPI: the tile epilogue has extra operands (accumulate into old dx and / or a residual addend): rare, so the common
// variant compiles their loads and registers out.
// BIAS: the conv has a bias.  Its gradient is the sum of dy over the tile's own pixels: the compute role adds the centre
// values it loads for the weight gradient (halo pixels belong to the neighbouring tiles, out-of-image slots hold zero),
// and slab row 9 carries the sums instead of zeros.  With a plain x (XMODE 0, ~200 VGPRs) the lane's eight running sums
// are registers.  With a prologue the bias-free kernel sits at the 256-register limit of two waves per SIMD and eight more
// accumulators spilled in its tile loop: there they live in two 16-byte LDS words of the lane's own, read, added to and
// written back once per tile (no contention, a fixed order).  Measured (profiles/ab_fused_bias.txt, HBM-cold, 16 x 256^2):
// the stems' 48-channel launch with a ReLU6 prologue 157.5 us against 155.2 for the bias-free kernel (208 with the spill,
// 228 with one LDS float atomic per sum and tile), the 32-channel one with a plain x 75.2 against 74.0; in the step
// 159 and 71 us (profiles/fused_bias_step.txt).  Nothing else depends on the bias: y is stored.  BIAS rides on the
// XMODE argument (XMODE_ = xmode | DW_BIAS): the bias-free instantiations keep their names and their code, and pay
// nothing for this.
constexpr int DW_BIAS = 4;
template <typename T, int YACT, int XMODE_, bool DB, bool EPI>
__global__ __launch_bounds__(DB ? 512 : 256) __attribute__((amdgpu_waves_per_eu(2, 2))) void dw_bn_bwd_kernel(FusedParams p) {
    constexpr int XMODE = XMODE_ & 3;
    constexpr bool BIAS = (XMODE_ & DW_BIAS) != 0;
    constexpr int PSD = dd_stride<T>::v;
    constexpr int XACT = XMODE == 1 ? ISA_ACT_RELU6 : (XMODE == 0 ? ISA_ACT_NONE : ACT_RT);
    constexpr int NBUF = DB ? 2 : 1;
    constexpr int NTHR = DB ? 512 : 256;
    constexpr int TILE_ELEMS = HALO * PSD;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    T* xt_base = reinterpret_cast<T*>(sm);                                   // [NBUF][HALO][PSD] RAW x (0 outside the image)
    T* dt_base = xt_base + NBUF * TILE_ELEMS;                                // [NBUF][HALO][PSD] dy
    float* wts = reinterpret_cast<float*>(dt_base + NBUF * TILE_ELEMS);      // [9][CB] flipped taps
    float* cst = wts + 9 * CB;                                               // [10][CB] per-channel constants
    float* red = cst + 10 * CB;                                              // [11*CB] (BIAS: [12*CB])
    f32x4* dbl = reinterpret_cast<f32x4*>(red + 12 * CB);                    // DB_LDS: [2][256] per-lane sums of dy
    constexpr bool DB_LDS = BIAS && XMODE != 0;
    const int tid = threadIdx.x;
    const int ltid = tid & 255;                                              // index inside the role group
    const bool loader = DB && tid >= 256;
    const int c_base = blockIdx.y * CB;
    const GroupSel gs = group_sel(p.G);
    if (gs.g) {                                                              // this workgroup's statistic group
        const long pix = (long)gs.g * p.n * p.h * p.w_, gc = (long)gs.g * p.c;
        p.g = reinterpret_cast<const T*>(p.g) + pix * p.ldg; p.y = reinterpret_cast<const T*>(p.y) + pix * p.ldy;
        p.x = reinterpret_cast<const T*>(p.x) + pix * p.ldx; p.dx = reinterpret_cast<T*>(p.dx) + pix * p.lddx;
        if (p.addend) p.addend = reinterpret_cast<const T*>(p.addend) + pix * p.lda;
        p.ysc += gc; p.ysh += gc; p.ymu += gc; p.yis += gc; p.yred += gc * ISA_STAT_R * 2;
        p.xsc = goff(p.xsc, gc); p.xsh = goff(p.xsh, gc); p.xmu = goff(p.xmu, gc); p.xis = goff(p.xis, gc);
        p.xred = goff(p.xred, gc * ISA_STAT_R * 2);
    }
    const int cg = ltid & 3, g4 = ltid >> 2, row = g4 >> 3, x0 = (g4 & 7) * 4;
    const int c0 = c_base + cg * 8;
    const bool cok = c0 < p.c;
    const T* wp = reinterpret_cast<const T*>(p.w);
    const T* gin = reinterpret_cast<const T*>(p.g);
    const T* yin = reinterpret_cast<const T*>(p.y);
    const T* xin = reinterpret_cast<const T*>(p.x);
    T* dxo = reinterpret_cast<T*>(p.dx);
    constexpr int NIT = (HALO * 4 + 255) / 256;
    constexpr int NB = 3;                            // single-buffer form: loads in chunks of 3 slots (registers)
    static_assert(NIT % NB == 0, "staging chunks");
    const bool want_xred = XMODE == 1 || (XMODE == 2 && p.xred != nullptr);

    // tile-invariant halo slot geometry (see dw2_fwd_kernel): per tile a scalar base per tensor and, on border tiles,
    // four scalar bounds
    int hrc[NIT], hog[NIT], hoy[NIT], hox[NIT];
    bool hok[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int pix = (ltid + it * 256) >> 2;
        const int rr = pix / (TW + 2), cc = pix - rr * (TW + 2);
        const int cc0 = cok ? c0 : c_base;
        hrc[it] = (rr << 16) | cc;
        hog[it] = (rr * p.w_ + cc) * p.ldg + cc0;
        hoy[it] = (rr * p.w_ + cc) * p.ldy + cc0;
        hox[it] = (rr * p.w_ + cc) * p.ldx + cc0;
        hok[it] = pix < HALO && cok;
    }
    const int oodx = (row * p.w_ + x0) * p.lddx + c0, ooa = (row * p.w_ + x0) * p.lda + c0;

    // ---- per-tile geometry shared by both staging forms
    struct Geo { const T *gb, *yb, *xb; int rlo, rhi, clo, chi, sg, sy, sx; bool interior; };
    auto geo = [&](int b, int ty, int tx) {
        Geo g;
        const long horg = ((long)b * p.h + ty * TH - 1) * p.w_ + tx * TW - 1;           // halo origin pixel (may lie outside)
        g.gb = gin + horg * p.ldg; g.yb = yin + horg * p.ldy; g.xb = xin + horg * p.ldx;
        g.rlo = 1 - ty * TH; g.rhi = p.h + 1 - ty * TH; g.clo = 1 - tx * TW; g.chi = p.w_ + 1 - tx * TW;
        g.interior = g.rlo <= 0 && g.rhi >= TH + 2 && g.clo <= 0 && g.chi >= TW + 2;
        const int cc0 = cok ? c0 : c_base;
        g.sg = (p.w_ + 1) * p.ldg + cc0; g.sy = (p.w_ + 1) * p.ldy + cc0; g.sx = (p.w_ + 1) * p.ldx + cc0;   // halo (1,1) = tile origin
        return g;
    };
    auto slot_ok = [&](const Geo& g, int it) {
        const int rr = hrc[it] >> 16, cc = hrc[it] & 0xffff;
        return hok[it] && (g.interior || (rr >= g.rlo && rr < g.rhi && cc >= g.clo && cc < g.chi));
    };
    // per-channel constants of the staging arithmetic: tile-invariant, so they live in registers for the whole kernel
    struct StageK { float sc[8], sh[8], mu[8], is[8], k0[8], k1[8]; };
    // one halo slot: dy = BN-backward(g, y) and raw x, both as storage type into the LDS tiles
    auto convert = [&](bool ok, int it, const StageK& K, const raw8<T>& gv, const raw8<T>& yv, const raw8<T>& xv, T* xt, T* dt) {
        const int pix = (ltid + it * 256) >> 2;
        if (pix >= HALO) return;
        float o[8];
        raw8<T> q = xv;                                           // raw x travels as it is: 16 bytes, no conversion
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float yy = yv.get(j);
            const float z = fmaf(yy, K.sc[j], K.sh[j]);
            const float dz = gv.get(j) * act_grad_t<YACT>(z, p.yact);
            const float yh = (yy - K.mu[j]) * K.is[j];
            o[j] = K.sc[j] * (dz - K.k0[j] - yh * K.k1[j]);
        }
        // out-of-image halo slots were fetched from the tile's origin pixel: zero them.  Interior tiles have none and the
        // test is uniform over the wave there, so the 16 selects are skipped
        if (__builtin_amdgcn_ballot_w64(!ok) != 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = ok ? o[j] : 0.f;
            if (!ok) q.zero();
        }
        store8<T>(dt + pix * PSD + cg * 8, o);
        q.store(xt + pix * PSD + cg * 8);
    };
    // Loads are unconditional (clamped address) so a chunk loop is straight-line code.  The empty asm keeps them where
    // they are written: LLVM otherwise sinks a prefetch down to its first use - across the LDS-only barrier and the loop
    // back-edge, into the `ok` branch - which undoes it and turns every partial vmcnt wait into a full one.
    auto issue = [&](const Geo& g, int it, raw8<T>& gv, raw8<T>& yv, raw8<T>& xv) {
        const bool ok = slot_ok(g, it);
        gv.load(g.gb + (ok ? hog[it] : g.sg));
        yv.load(g.yb + (ok ? hoy[it] : g.sy));
        xv.load(g.xb + (ok ? hox[it] : g.sx));
        asm volatile("" ::: "memory");
    };

    // ---- launch prologue, one round trip: the loader role's first tile is the kernel's first memory traffic; the
    // weights, the BN(y) constants with their replica sums and the BN(x) constants are requested behind it, every one
    // unconditionally (a null optional pointer selects ysc, which always exists, and its value is replaced by the
    // neutral constant), and waited for once, ahead of the single barrier.  (Conditional loads, each with its own full
    // wait, and the tile loads behind the barrier made this about seven dependent trips.)
    TileIter tn;                                                 // loader: the tile whose loads are in flight
    raw8<T> gv[NIT], yv[NIT], xv[NIT];
    Geo gn;
    if constexpr (DB) {
        if (loader) {
            tn.init(tile_range(p.ntiles, gs.bx, gs.nbx), p.tiles_x, p.tiles_y);
            if (tn.valid()) {
                gn = geo(tn.b, tn.ty, tn.tx);
#pragma unroll
                for (int it = 0; it < NIT; ++it) issue(gn, it, gv[it], yv[it], xv[it]);
            }
        }
    }
    constexpr int NW = (9 * CB + NTHR - 1) / NTHR;
    float wv[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int i = min(tid + k * NTHR, 9 * CB - 1);
        const int tp = i / CB, cc = i - tp * CB;
        wv[k] = st<T>::ld(wp + (long)tp * p.wld + min(c_base + cc, p.c - 1));
    }
    if (tid < CB) {
        const int c = min(c_base + tid, p.c - 1);
        const bool hsc = XMODE && p.xsc, hsh = XMODE && p.xsh, hmu = XMODE && p.xmu, his = XMODE && p.xis;
        const float ysc = p.ysc[c], ysh = p.ysh[c], ymu = p.ymu[c], yis = p.yis[c];
        float ra[ISA_STAT_R], rb[ISA_STAT_R];
#pragma unroll
        for (int r = 0; r < ISA_STAT_R; ++r) { ra[r] = p.yred[r * 2 * p.c + c]; rb[r] = p.yred[r * 2 * p.c + p.c + c]; }
        float xsc = 1.f, xsh = 0.f, xmu = 0.f, xis = 1.f;
        if constexpr (XMODE != 0) {
            xsc = (hsc ? p.xsc : p.ysc)[c]; xsh = (hsh ? p.xsh : p.ysc)[c];
            xmu = (hmu ? p.xmu : p.ysc)[c]; xis = (his ? p.xis : p.ysc)[c];
        }
        asm volatile("" ::: "memory");
        cst[0 * CB + tid] = ysc; cst[1 * CB + tid] = ysh; cst[2 * CB + tid] = ymu; cst[3 * CB + tid] = yis;
        float r0 = 0.f, r1 = 0.f;                                // fold the ISA_STAT_R replicas of BN(y)'s backward sums
#pragma unroll
        for (int r = 0; r < ISA_STAT_R; ++r) { r0 += ra[r]; r1 += rb[r]; }
        cst[4 * CB + tid] = r0 * p.ycnt_inv; cst[5 * CB + tid] = r1 * p.ycnt_inv;
        cst[6 * CB + tid] = hsc ? xsc : 1.f; cst[7 * CB + tid] = hsh ? xsh : 0.f;
        cst[8 * CB + tid] = hmu ? xmu : 0.f; cst[9 * CB + tid] = his ? xis : 1.f;
        if (gs.bx == 0 && c_base + tid < p.c) {                  // BN(y) parameter gradients: dbeta = sum g', dgamma = sum g'*yhat (per group)
            if (p.ydgamma) atomicAdd(p.ydgamma + c, r1);
            if (p.ydbeta) atomicAdd(p.ydbeta + c, r0);
        }
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int i = tid + k * NTHR;
        if (i < 9 * CB) wts[i] = (c_base + (i & (CB - 1)) < p.c) ? wv[k] : 0.f;
    }
    for (int i = tid; i < (11 + BIAS) * CB; i += NTHR) red[i] = 0.f;     // rows 0-8: dW taps, 9-10: BN(x) sums (BIAS: 11 = sum dy)

    // single-buffer form: one tile, chunks of NB slots
    auto stage = [&](int b, int ty, int tx, T* xt, T* dt) {
        const Geo g = geo(b, ty, tx);
        StageK K;                                                 // per tile here: these threads also hold the accumulators
        ld8(cst + 0 * CB + cg * 8, K.sc); ld8(cst + 1 * CB + cg * 8, K.sh); ld8(cst + 2 * CB + cg * 8, K.mu);
        ld8(cst + 3 * CB + cg * 8, K.is); ld8(cst + 4 * CB + cg * 8, K.k0); ld8(cst + 5 * CB + cg * 8, K.k1);
#pragma unroll
        for (int it0 = 0; it0 < NIT; it0 += NB) {
            raw8<T> gv[NB], yv[NB], xv[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) issue(g, it0 + u, gv[u], yv[u], xv[u]);
#pragma unroll
            for (int u = 0; u < NB; ++u) convert(slot_ok(g, it0 + u), it0 + u, K, gv[u], yv[u], xv[u], xt, dt);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    float db[BIAS && !DB_LDS ? 8 : 1];                           // BIAS: sum of dy over this lane's centre pixels (compute role)
#pragma unroll
    for (int j = 0; j < (BIAS && !DB_LDS ? 8 : 1); ++j) db[j] = 0.f;
    if constexpr (DB_LDS) {
        if (!loader) { dbl[ltid] = f32x4{0.f, 0.f, 0.f, 0.f}; dbl[256 + ltid] = f32x4{0.f, 0.f, 0.f, 0.f}; }     // this lane's own words
    }
    auto compute = [&](int b, int ty, int tx, const T* xt, const T* dt, float (&acc)[9][8], float (&s0)[8], float (&s1)[8]) {
        const long torg = ((long)b * p.h + ty * TH) * p.w_ + tx * TW;                      // tile origin pixel
        T* dxb = dxo + torg * p.lddx + oodx;
        const T* adb = reinterpret_cast<const T*>(p.addend) + torg * p.lda + ooa;
        const bool rowok = ty * TH + row < p.h && cok;
        const int xlim = p.w_ - tx * TW;                                                   // x0 + o < xlim
        // rare epilogue operands (old dx for accumulate, the residual addend): requested before the stencil
        raw8<T> oc[4], ad[4];
        if constexpr (EPI) {
            if (rowok) {
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    if (x0 + o >= xlim) continue;
                    if (p.accumulate) oc[o].load(dxb + o * p.lddx);
                    if constexpr (XMODE == 0) { if (p.addend) ad[o].load(adb + o * p.lda); }
                }
            }
        }
        {   // ---- data gradient: dx tile = flipped taps over dy (halo), then BN(x)-backward sums
            float a[4][8];
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int j = 0; j < 8; ++j) a[o][j] = 0.f;
#pragma unroll 1
            for (int dy = 0; dy < 3; ++dy) {
                float wr[3][8], in[6][8];
#pragma unroll
                for (int k = 0; k < 3; ++k) ld8(wts + (dy * 3 + k) * CB + cg * 8, wr[k]);
#pragma unroll
                for (int k = 0; k < 6; ++k) load8<T>(dt + ((row + dy) * (TW + 2) + x0 + k) * PSD + cg * 8, in[k]);
#pragma unroll
                for (int o = 0; o < 4; ++o)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        fma8(in[o + k], wr[k], a[o]);
            }
            if (rowok) {
                float xs[8], xh[8], xm[8], xi[8];
                if (want_xred) {
                    ld8(cst + 6 * CB + cg * 8, xs); ld8(cst + 7 * CB + cg * 8, xh);
                    ld8(cst + 8 * CB + cg * 8, xm); ld8(cst + 9 * CB + cg * 8, xi);
                }
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    if (x0 + o >= xlim) continue;
                    T* dst = dxb + o * p.lddx;
                    if constexpr (EPI) {
                        if (p.accumulate) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) a[o][j] += oc[o].get(j);
                        }
                        if constexpr (XMODE == 0) {          // plain-tensor input: the only case with a residual branch
                            if (p.addend) {
#pragma unroll
                                for (int j = 0; j < 8; ++j) a[o][j] += ad[o].get(j);
                            }
                        }
                    }
                    store8<T>(dst, a[o]);
                    if (want_xred) {
                        // the unfused reduce reads the stored (rounded) gradient: round the same way
                        float xr[8];
                        load8<T>(xt + ((row + 1) * (TW + 2) + x0 + 1 + o) * PSD + cg * 8, xr);      // raw x, centre pixel
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float gq = (float)(T)a[o][j];
                            const float z = fmaf(xr[j], xs[j], xh[j]);
                            const float dz = gq * act_grad_t<XACT>(z, p.xact);
                            s0[j] += dz; s1[j] += dz * ((xr[j] - xm[j]) * xi[j]);
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        {   // ---- weight gradient: 9 x 8 products per lane, dy centre x pro(x) window
            float d[4][8];
#pragma unroll
            for (int o = 0; o < 4; ++o) load8<T>(dt + ((row + 1) * (TW + 2) + x0 + 1 + o) * PSD + cg * 8, d[o]);
            if constexpr (DB_LDS) {
                f32x4 lo = dbl[ltid], hi = dbl[256 + ltid];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lo[j] += (d[0][j] + d[1][j]) + (d[2][j] + d[3][j]);
                    hi[j] += (d[0][4 + j] + d[1][4 + j]) + (d[2][4 + j] + d[3][4 + j]);
                }
                dbl[ltid] = lo; dbl[256 + ltid] = hi;
            } else if constexpr (BIAS) {
#pragma unroll
                for (int j = 0; j < 8; ++j) db[j] += (d[0][j] + d[1][j]) + (d[2][j] + d[3][j]);
            }
            float ps[8], ph[8];
            if constexpr (XMODE != 0) { ld8(cst + 6 * CB + cg * 8, ps); ld8(cst + 7 * CB + cg * 8, ph); }
            // Zero padding applies to pro(x), not to x: on border tiles the out-of-image window slots are masked after
            // the prologue.  Two copies of the stencil behind a uniform branch - as one body with per-slot predicates
            // the 18 lane masks stayed live across the loop and the accumulators spilled.
            const int rlo = 1 - ty * TH, rhi = p.h + 1 - ty * TH, clo = 1 - tx * TW, chi = p.w_ + 1 - tx * TW;
            const bool interior = XMODE == 0 || (rlo <= 0 && rhi >= TH + 2 && clo <= 0 && chi >= TW + 2);
            auto window = [&](auto border) {
                constexpr bool BORDER = decltype(border)::value;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const bool row_in = row + dy >= rlo && row + dy < rhi;
#pragma unroll
                    for (int k = 0; k < 6; ++k) {                // one window pixel at a time: 8 live registers, not 48
                        float in[8];
                        load8<T>(xt + ((row + dy) * (TW + 2) + x0 + k) * PSD + cg * 8, in);
                        if constexpr (XMODE != 0) {
                            float z[8];
#pragma unroll
                            for (int j = 0; j < 8; ++j) z[j] = ph[j];
                            fma8(in, ps, z);                     // packed fma; the clamp has no packed form
#pragma unroll
                            for (int j = 0; j < 8; ++j) in[j] = act_t<XACT>(z[j], p.xact);
                            if constexpr (BORDER) {
                                const bool in_img = row_in && x0 + k >= clo && x0 + k < chi;
#pragma unroll
                                for (int j = 0; j < 8; ++j) in[j] = in_img ? in[j] : 0.f;
                            }
                        }
#pragma unroll
                        for (int o = 0; o < 4; ++o)
                            if (k - o >= 0 && k - o < 3) fma8(in, d[o], acc[dy * 3 + (k - o)]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            if (interior) window(std::false_type{});
            else window(std::true_type{});
        }
    };

    // The accumulators exist only on the compute side of the role split, so the register allocator sees
    // max(loader set, compute set) instead of their sum.  Both sides execute the same number of barriers.
    __syncthreads();                                             // constants + zeroed `red` visible
    if (loader) {
        // Software-pipelined across tiles: the loads of the tile after next are issued chunk by chunk WHILE the next tile
        // is converted - a chunk's registers are refilled right after its arithmetic consumed them, so a tile's worth of
        // 16-byte loads (3 x NIT per lane) is always in flight and a chunk only waits for loads issued a tile earlier.
        // Barriers: one per staged tile (the first is the compute side's "first tile staged", every later one closes the
        // compute side's previous tile) plus one closing its last tile: n + 1 on both sides.  The steady branch is
        // straight-line code with the same loads in flight at its top and bottom, so its vmcnt waits stay partial.
        StageK K;
        ld8(cst + 0 * CB + cg * 8, K.sc); ld8(cst + 1 * CB + cg * 8, K.sh); ld8(cst + 2 * CB + cg * 8, K.mu);
        ld8(cst + 3 * CB + cg * 8, K.is); ld8(cst + 4 * CB + cg * 8, K.k0); ld8(cst + 5 * CB + cg * 8, K.k1);
        // (the first tile's loads were issued in the launch prologue)
        Geo gs;
        bool have = tn.valid();
        int buf = 0;
        while (have) {
            gs = gn;
            tn.next();
            T* xt = xt_base + buf * TILE_ELEMS; T* dt = dt_base + buf * TILE_ELEMS;
            if (tn.valid()) {
                gn = geo(tn.b, tn.ty, tn.tx);
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    convert(slot_ok(gs, it), it, K, gv[it], yv[it], xv[it], xt, dt);
                    issue(gn, it, gv[it], yv[it], xv[it]);         // refill the chunk's registers: the tile after this one
                }
            } else {
#pragma unroll
                for (int it = 0; it < NIT; ++it) convert(slot_ok(gs, it), it, K, gv[it], yv[it], xv[it], xt, dt);
                have = false;
            }
            lds_barrier();
            buf ^= 1;
        }
        lds_barrier();
    } else {
        float acc[9][8], s0[8], s1[8];
#pragma unroll
        for (int tp = 0; tp < 9; ++tp)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[tp][j] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { s0[j] = 0.f; s1[j] = 0.f; }
        if constexpr (DB) {
            TileIter ti; ti.init(tile_range(p.ntiles, gs.bx, gs.nbx), p.tiles_x, p.tiles_y);
            int buf = 0;
            lds_barrier();                                       // first tile staged
            for (; ti.valid(); ti.next()) {
                compute(ti.b, ti.ty, ti.tx, xt_base + buf * TILE_ELEMS, dt_base + buf * TILE_ELEMS, acc, s0, s1);
                lds_barrier();
                buf ^= 1;
            }
        } else {
            TileIter ti; ti.init(TileRange{(long)gs.bx, p.ntiles, (long)gs.nbx}, p.tiles_x, p.tiles_y);
            for (; ti.valid(); ti.next()) {
                stage(ti.b, ti.ty, ti.tx, xt_base, dt_base);
                __syncthreads();
                compute(ti.b, ti.ty, ti.tx, xt_base, dt_base, acc, s0, s1);
                __syncthreads();                                 // tile fully consumed before it is restaged
            }
        }
        // Fold this lane's 88 sums WITHOUT atomics (a phase trace of a one-tile launch: 26 k of its 47 k cycles sat in the
        // old fold - a ds_bpermute tree per value plus same-address LDS float atomics from four waves).  Row sums by
        // DPP, then the 16 rows of the 4 compute waves park their partials in the (now idle) tile buffers:
        // part[(v * 4 + cg) * 16 + wave * 4 + row]; 352 threads add 16 partials each after the barrier below.
        float* part = reinterpret_cast<float*>(sm);
        const int slot = cg * 16 + (tid >> 6) * 4 + ((tid >> 4) & 3);
        const bool writer = (tid & 15) < 4;
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = row_fold<4>(acc[tp][j]);
                if (writer) part[(tp * 8 + j) * 64 + slot] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v0 = row_fold<4>(s0[j]), v1 = row_fold<4>(s1[j]);
            if (writer) { part[(72 + j) * 64 + slot] = v0; part[(80 + j) * 64 + slot] = v1; }
        }
        if constexpr (BIAS) {
            float dv[8];
            if constexpr (DB_LDS) {
                const f32x4 lo = dbl[ltid], hi = dbl[256 + ltid];
#pragma unroll
                for (int j = 0; j < 4; ++j) { dv[j] = lo[j]; dv[4 + j] = hi[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) dv[j] = db[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = row_fold<4>(dv[j]);
                if (writer) part[(88 + j) * 64 + slot] = v;
            }
        }
    }
    __syncthreads();
    {
        const float* part = reinterpret_cast<const float*>(sm);
        for (int o = tid; o < (88 + 8 * BIAS) * 4; o += NTHR) {  // o = v * 4 + cg
            const f32x4 a = *reinterpret_cast<const f32x4*>(part + o * 16), b = *reinterpret_cast<const f32x4*>(part + o * 16 + 4),
                        c = *reinterpret_cast<const f32x4*>(part + o * 16 + 8), d = *reinterpret_cast<const f32x4*>(part + o * 16 + 12);
            const f32x4 t = (a + b) + (c + d);
            const int v = o >> 2, g = o & 3;
            red[(v >> 3) * CB + g * 8 + (v & 7)] = (t[0] + t[1]) + (t[2] + t[3]);
        }
    }
    __syncthreads();
    float* slab = p.ws + ((long)blockIdx.x * gridDim.y + blockIdx.y) * 10 * CB;
    if constexpr (BIAS) {
        for (int i = tid; i < 10 * CB; i += NTHR) slab[i] = i < 9 * CB ? red[i] : red[i + 2 * CB];     // row 9 = conv bias slot: sum dy
    } else {
        for (int i = tid; i < 10 * CB; i += NTHR) slab[i] = i < 9 * CB ? red[i] : 0.f;       // row 9 = conv bias slot (none here)
    }
    if (want_xred && tid < 2 * CB) {
        const int cc = tid & (CB - 1), which = tid / CB;
        const float v = red[9 * CB + tid];
        if (c_base + cc < p.c && v != 0.f) {
            float* rep = p.xred + ((blockIdx.x + blockIdx.y) & (ISA_STAT_R - 1)) * 2 * p.c;
            atomicAdd(rep + which * p.c + c_base + cc, v);
        }
    }
}

template <typename T, int YACT, int XMODE, bool BIAS, bool EPI = true>
int launch_fused_inst(FusedParams& p, dim3 grid, hipStream_t s) {
    constexpr bool DB = sizeof(T) == 2;                          // two pairs of tile buffers: 109 KB for bf16, 196 KB for f32
    if constexpr (EPI) {
        if (!p.accumulate && !p.addend) return launch_fused_inst<T, YACT, XMODE, BIAS, false>(p, grid, s);
    }
    constexpr int NBUF = DB ? 2 : 1;
    constexpr size_t lds = NBUF * 2 * (size_t)HALO * dd_stride<T>::v * sizeof(T) + (9 + 10 + 11 + BIAS) * CB * 4 + BIAS * 8 * 256 * 4;   // raw x + dy tiles
    constexpr auto kern = &dw_bn_bwd_kernel<T, YACT, XMODE | (BIAS ? DW_BIAS : 0), DB, EPI>;
    static bool configured = false;
    if (!configured) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return ISA_ELAUNCH;
        configured = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(DB ? 512 : 256), lds, s, p);
    return launch_status();
}

template <typename T>
int launch_fused(FusedParams& p, float* dbias, int xmode, long ws_floats, isa_slab_arena* sa, const isa_pro* xfin, int xfin_groups, hipStream_t s) {
    set_tiles(p);
    const int ncb = (p.c + CB - 1) / CB;
    long gx;                             // 1 resident workgroup per CU.  LDS: 156 KB (bf16, double-buffered) / 100 KB (f32)
    if (int rc = slab_plan(sa, &p.ws, ws_floats, want_grid(p, 256L, ncb), 10L * CB * ncb, p.G, &gx)) return rc;
    dim3 grid((unsigned)gx, ncb);
    if (int rc = fin_standalone(xfin, p.c, xfin_groups, s)) return rc;         // every check has passed
    const int rc = by_flag(dbias != nullptr, [&](auto b) { return by_int<ISA_ACT_RELU6, ACT_RT>(p.yact, [&](auto ya) {
        return by_int<0, 1, 2>(xmode, [&](auto xm) {
            return launch_fused_inst<T, decltype(ya)::value, decltype(xm)::value, decltype(b)::value>(p, grid, s);
        }); }); });
    if (rc != ISA_OK) return rc;
    return dw_slab_reduce_launch(p.ws, p.dw, dbias, (int)gx, ncb, CB, p.c, p.csrc, sa, s);
}

// forward, and the data gradient as the forward of dy
int dw_forward(const isa_tensor* x, const isa_pro* pro, const void* w, const float* bias, const isa_tensor* y,
               float* stats, int accumulate, void* stream) {
    if (!tensor_ok(x, 8) || !tensor_ok(y, 8) || !w || x->dtype != y->dtype) return ISA_EINVAL;
    if (x->n != y->n || x->h != y->h || x->w != y->w || x->c != y->c) return ISA_EINVAL;
    Dw2Params p{};
    p.x = x->data; p.w = w; p.bias = bias; p.y = y->data;
    p.n = x->n; p.h = x->h; p.w_ = x->w; p.c = x->c; p.ldx = x->ld; p.ldy = y->ld; p.wld = ((x->c + 7) / 8) * 8;
    p.pro = make_pro(pro); p.stats = stats; p.accumulate = accumulate;
    const bool has_pro = !pro_trivial(p.pro);
    p.G = stat_groups(x, stats || p.pro.scale || p.pro.shift);
    if (!p.G || (p.G > 1 && tensor_groups(y) != p.G)) return ISA_EINVAL;
    p.n = x->n / p.G;
    if (pro && pro->fin) {
        if (!fin_valid(pro)) return ISA_EINVAL;
        p.fin = make_fin(pro);
    }
    return by_dtype(x->dtype, [&](auto t) { return launch_fwd2<decltype(t)>(p, has_pro, as_stream(stream)); });
}

}  // namespace

extern "C" int isa_dwconv3x3(const isa_tensor* x, const isa_pro* pro, const void* w,
                             const float* bias, const isa_tensor* y, float* stats, void* stream) {
    return dw_forward(x, pro, w, bias, y, stats, 0, stream);
}

// w must be the tap-flipped packing of the forward weights (isa_pack_weights kind 5)
extern "C" int isa_dwconv3x3_dgrad(const isa_tensor* dy, const void* w, const isa_tensor* dx,
                                   int32_t accumulate, void* stream) {
    return dw_forward(dy, nullptr, w, nullptr, dx, nullptr, accumulate, stream);
}

extern "C" int isa_dwconv3x3_wgrad(const isa_tensor* x, const isa_pro* pro, const isa_tensor* dy,
                                   float* dw, float* dbias, int32_t csrc, float* ws, int64_t ws_floats, isa_slab_arena* defer,
                                   void* stream) {
    if (!tensor_ok(x, 8) || !tensor_ok(dy, 8) || !dw || x->dtype != dy->dtype) return ISA_EINVAL;
    if (x->n != dy->n || x->h != dy->h || x->w != dy->w || x->c != dy->c) return ISA_EINVAL;
    if (!ws && !defer) return ISA_EINVAL;
    if (!fin_valid(pro)) return ISA_EINVAL;        // a pending finalize (no in-kernel form here) runs after the last check
    Dw2Params p{};
    p.x = x->data; p.dy = dy->data; p.y = dw; p.bias = dbias;        // y/bias slots carry the output pointers
    p.n = x->n; p.h = x->h; p.w_ = x->w; p.c = x->c; p.ldx = x->ld; p.ldd = dy->ld;
    p.pro = make_pro(pro); p.ws = ws; p.csrc = (csrc > 0 && csrc < x->c) ? csrc : x->c;
    const bool has_pro = !pro_trivial(p.pro);
    p.G = stat_groups(x, p.pro.scale || p.pro.shift);
    if (!p.G) return ISA_EINVAL;
    p.n = x->n / p.G;
    return by_dtype(x->dtype, [&](auto t) { return launch_wg2<decltype(t)>(p, has_pro, ws_floats, defer, pro, as_stream(stream)); });
}

// Fused BN-apply + depthwise dgrad/wgrad + next BN-reduce; see dw_bn_bwd_kernel.  dbias (optional): the conv's bias gradient
extern "C" int isa_dwconv3x3_bias_bn_backward(const isa_tensor* g, const isa_tensor* y, const isa_bn_bwd* ybn,
                                              const isa_tensor* x, const isa_pro* xpro, const isa_bn_bwd* xbn,
                                              const void* w_flipped, float* dw, int32_t csrc,
                                              const isa_tensor* dx, int32_t accumulate, const isa_tensor* addend,
                                              float* ws, int64_t ws_floats, isa_slab_arena* defer, void* stream,
                                              float* dbias) {
    if (!tensor_ok(g, 8) || !tensor_ok(y, 8) || !tensor_ok(x, 8) || !tensor_ok(dx, 8)) return ISA_EINVAL;
    if (!fin_valid(xpro)) return ISA_EINVAL;      // a pending finalize (no in-kernel form here) runs after the last check
    if (!bn_bwd_ok(ybn) || !xbn_ok(xbn)) return ISA_EINVAL;
    if (!w_flipped || !dw || (!ws && !defer)) return ISA_EINVAL;
    if (x->c % 8 != 0) return ISA_EINVAL;
    const isa_tensor* ts[3] = {y, x, dx};
    for (const isa_tensor* t : ts)
        if (t->n != g->n || t->h != g->h || t->w != g->w || t->c != g->c || t->dtype != g->dtype) return ISA_EINVAL;
    const ProDev xp = make_pro(xpro);
    if (xp.bscale) return ISA_EINVAL;                             // per-image scales are not folded here
    // an addend only next to a plain-tensor x
    if (addend && (!addend_ok(addend, g, g->c) || !pro_trivial(xp) || xbn)) return ISA_EINVAL;
    FusedParams p{};
    p.g = g->data; p.y = y->data; p.x = x->data; p.w = w_flipped; p.dx = dx->data;
    p.n = g->n; p.h = g->h; p.w_ = g->w; p.c = g->c; p.ldg = g->ld; p.ldy = y->ld; p.ldx = x->ld; p.lddx = dx->ld;
    p.wld = ((g->c + 7) / 8) * 8;
    set_bn_bwd(p, ybn, xp, xbn);
    p.accumulate = accumulate; p.ws = ws; p.dw = dw;
    if (addend) { p.addend = addend->data; p.lda = addend->ld; }
    p.csrc = (csrc > 0 && csrc < g->c) ? csrc : g->c;
    p.G = stat_groups(g, true);                                      // BN(y) constants and sums are per statistic group
    if (!p.G) return ISA_EINVAL;
    p.n = g->n / p.G;
    return by_dtype(g->dtype, [&](auto t) {
        return launch_fused<decltype(t)>(p, dbias, fused_xmode(xp, xbn), ws_floats, defer, xpro, tensor_groups(x), as_stream(stream));
    });
}

extern "C" int isa_dwconv3x3_bn_backward(const isa_tensor* g, const isa_tensor* y, const isa_bn_bwd* ybn,
                                         const isa_tensor* x, const isa_pro* xpro, const isa_bn_bwd* xbn,
                                         const void* w_flipped, float* dw, int32_t csrc,
                                         const isa_tensor* dx, int32_t accumulate, const isa_tensor* addend,
                                         float* ws, int64_t ws_floats, isa_slab_arena* defer, void* stream) {
    return isa_dwconv3x3_bias_bn_backward(g, y, ybn, x, xpro, xbn, w_flipped, dw, csrc, dx, accumulate, addend, ws, ws_floats,
                                          defer, stream, nullptr);
}
