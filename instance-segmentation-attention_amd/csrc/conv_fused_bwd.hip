// Fused backward of   x --1x1 conv (W[N][K])--> y --BN(train)(+act)--> ...   for bf16 storage and N, K <= 64:
//     dy   = BN-backward(g, y)                         (isa_bn_bwd_apply, never stored)
//     dW  += dy^T . pro(x)                             (isa_conv_wgrad)
//     dx (+)= dy . W                                   (isa_conv_gemm data gradient)
//     xbn:  sums of BN(x)'s backward over the finished dx   (isa_bn_bwd_reduce of the layer that made x)
// in ONE pass: reads g, y, x once and writes dx once (6 narrow-tensor passes instead of 12-13).  With y == NULL (REC) y is
// not read either: the wave recomputes its 32 x N tile from the pro(x) slab and W, bit for bit what isa_conv_gemm stored.
//
// Built on the bf16 weight-gradient kernel's structure (conv_wgrad.hip): every WAVE owns 32-pixel chunks,
// staged row-major in a wave-private LDS slab; no __syncthreads in the main loop; the next chunk's raw
// 16-byte loads are in flight while the current chunk's MFMAs run (the BN/ReLU6 arithmetic is done when the
// registers are stashed to LDS, not when they are fetched).  The first chunk's loads leave before the weights and the
// constants are staged, and the four waves' weight-gradient fragments are folded in one parallel pass (tr_lds.hpp).
//   wgrad:  dW[n][k] += sum_px dy[px][n] x[px][k]   A/B fragments by ds_read_b64_tr_b16 (pixel-contraction)
//   dgrad:  dx[px][k] = sum_n  dy[px][n] W[n][k]    A = ds_read_b128 rows of the SAME dy slab,
//                                                    B = W fragments held in registers for the whole kernel
//   the 32xK dx tile goes through the x slab (bf16) so global stores are 16-byte row pieces.
#include "common.hpp"
#include "tr_lds.hpp"

namespace {

struct PwParams {
    const bf16_t *g, *y, *x; bf16_t* dx; const float* w; float* dw;
    int N, K, ldg, ldy, ldx, lddx; long M;
    const float *ysc, *ysh, *ymu, *yis, *yred; float ycnt_inv; int yact; float *ydgamma, *ydbeta;
    const float *xsc, *xsh, *xmu, *xis; int xact; float* xred;
    int accumulate; float* ws;
    const bf16_t* addend; int lda;       // optional: dx += addend (the residual branch's gradient, saves its axpy pass)
    int G;                               // statistic groups: M is per group (common.hpp)
};
constexpr int PW_BIAS = 4;               // flag on the kernel's XMODE_ argument: the conv has a bias
// The y slot of the argument block in the biased recompute instantiations (REC && BIAS): REC never reads y, and there
// the slot holds the conv's fp32 bias vector instead.  These two functions are the only places that say so; kernel code
// that wants the bias calls rec_bias<REC, BIAS>(p) and fails to compile in any other instantiation.
template <bool REC, bool BIAS>
__host__ __device__ __forceinline__ const float* rec_bias(const PwParams& p) {
    static_assert(REC && BIAS, "the y slot carries the bias vector in the biased recompute instantiations only");
    return reinterpret_cast<const float*>(p.y);
}
template <bool REC, bool BIAS>
inline void set_rec_bias(PwParams& p, const float* bias) {
    static_assert(REC && BIAS, "the y slot carries the bias vector in the biased recompute instantiations only");
    p.y = reinterpret_cast<const bf16_t*>(bias);
}

#ifdef ISA_PHASE_TRACE
__device__ unsigned long long phase_buf[10];
#endif

// dy of one element: BN(y)'s backward (isa_bn_bwd_apply) with q = invstd * mean(g' yhat) and k0 = mean(g').  The recompute
// variant's form of the expression that the stored-y stash spells out: same operations in the same order
template <int YACT>
__device__ __forceinline__ float bn_bwd_dy(float g, float yy, float sc, float sh, float mu, float q, float k0, int rt) {
    const float dz = g * act_grad_t<YACT>(fmaf(yy, sc, sh), rt);
    return sc * (dz - k0 - (yy - mu) * q);
}

// tr_frag (tr_lds.hpp) with the half-waves HS rows apart: element j of lane (r, h) <- tile[row0 + HS h + j][col0 + r]
template <int HS>
__device__ __forceinline__ bf16x8 tr_frag_h(const char* tile, int stride_bytes, int row0, int col0, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, pp = i & 3;
    const char* a = tile + (row0 + HS * (g >> 1) + q) * stride_bytes + (col0 + 16 * (g & 1) + 4 * pp) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(a));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(a + 4 * stride_bytes));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// W fragment of the recompute's contraction step s (see wf in the kernel) for the 32-channel tile i, from the [k][n] staging
template <int WP>
__device__ __forceinline__ bf16x8 rec_wfrag(const bf16_t* wl, int s, int i, int lane) {
    return tr_frag_h<16>(reinterpret_cast<const char*>(wl), WP * 2, 32 * (s >> 1) + 8 * (s & 1), i * 32, lane);
}

// XMODE 0: plain x; 1: x = relu6(scale*x+shift) with BN(x) sums produced; 2: runtime prologue, sums if p.xred
// EPI: the store epilogue adds the old dx and / or the residual addend (p.accumulate, p.addend); without it their
// loads and the waits that go with them are compiled out
// REC: y is not read but recomputed per chunk as W . pro(x) from the pro(x) slab and register-held W fragments, with the
// forward kernel's MFMA sequence (conv_gemm.hip, conv_gemm_kernel) so that the rounded bf16 value is the one it stored;
// raw g waits in the dy slab and is overwritten by dy in the accumulator layout
// BIAS: the conv has a bias.  The recompute adds it where the forward's epilogue does (fp32, before the bf16 rounding), and
// lane (r, hh) sums the dy values of its 16 pixels of channel 32 i + r as the dy slab holds them (rounded and masked): the
// slab's bias slot carries the workgroup's column sums of dy instead of zeros.  The stored-y form reads them back from
// the slab in the recompute's layout and order, so both forms give the same bits.  Without BIAS all of this is compiled out.
// BIAS rides on the XMODE argument (XMODE_ = xmode | PW_BIAS) and the recompute finds the bias vector in the y slot, which
// it does not use otherwise: the bias-free instantiations keep their names, their argument block and their code
template <int TN, int TK, int YACT, int XMODE_, bool EPI, bool REC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void pw_bn_bwd_kernel(PwParams p) {
    constexpr int XMODE = XMODE_ & 3;
    constexpr bool BIAS = (XMODE_ & PW_BIAS) != 0;
    extern __shared__ __attribute__((aligned(16))) char ldsb[];
    PHASE_DECL(); PHASE(0);
    constexpr int PMB = 32;
    constexpr int SN = TrStride<TN * 32>::bytes, SK = TrStride<TK * 32>::bytes;
    constexpr int SLAB = PMB * (SN + SK);
    constexpr int VN = TN * 4, VK = TK * 4;
    constexpr int LOADS_N = PMB * VN / 64, LOADS_K = PMB * VK / 64;
    constexpr int RPN = 64 / VN, RPK = 64 / VK;
    constexpr int XACT = XMODE == 1 ? ISA_ACT_RELU6 : (XMODE == 0 ? ISA_ACT_NONE : ACT_RT);
    constexpr int NS = TN * 2;                                   // 16-wide contraction steps over N (data gradient)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 31, hh = lane >> 5;
    char* sD = ldsb + wave * SLAB;
    char* sX = sD + PMB * SN;
    const GroupSel gs = group_sel(p.G);
    if (gs.g) {                                                  // this workgroup's statistic group: rows [g*M, (g+1)*M)
        const long gm = (long)gs.g * p.M;
        p.g += gm * p.ldg;
        if constexpr (!REC) p.y += gm * p.ldy;
        p.x += gm * p.ldx; p.dx += gm * p.lddx;
        if (p.addend) p.addend += gm * p.lda;
        p.ysc += gs.g * p.N; p.ysh += gs.g * p.N; p.ymu += gs.g * p.N; p.yis += gs.g * p.N; p.yred += gs.g * ISA_STAT_R * 2 * p.N;
        p.xsc = goff(p.xsc, (long)gs.g * p.K); p.xsh = goff(p.xsh, (long)gs.g * p.K); p.xmu = goff(p.xmu, (long)gs.g * p.K);
        p.xis = goff(p.xis, (long)gs.g * p.K); p.xred = goff(p.xred, (long)gs.g * ISA_STAT_R * 2 * p.K);
    }
    const bool want_xred = XMODE == 1 || (XMODE == 2 && p.xred != nullptr);

    // ---- per-lane constants: a lane keeps ONE 8-channel group of each operand
    const int cgn = lane % VN, rown = lane / VN, cgk = lane % VK, rowk = lane / VK;
    const int cn0 = cgn * 8, ck0 = cgk * 8;
    const bool nok = cn0 < p.N, kok = ck0 < p.K;
    const int cnl = nok ? cn0 : 0, ckl = kok ? ck0 : 0;           // clamped: a 16-byte piece that exists in every row

    bf16x8 rg[LOADS_N], ry[REC ? 1 : LOADS_N], rx[LOADS_K], rxc[LOADS_K];
    const long nchunks = (p.M + PMB - 1) / PMB;
    // raw 16-byte loads only, for EVERY lane at a clamped address and with no branch in front: nothing here waits on
    // memory, and the number of loads in flight is the same on every path.  stash() zeroes what lies past M, N or K.
    auto fetch = [&](long chunk) {
        const long mbase = chunk * PMB;
#pragma unroll
        for (int v = 0; v < LOADS_N; ++v) {
            const long m = min(mbase + v * RPN + rown, p.M - 1);
            rg[v] = *reinterpret_cast<const bf16x8*>(p.g + m * p.ldg + cnl);
            if constexpr (!REC) ry[v] = *reinterpret_cast<const bf16x8*>(p.y + m * p.ldy + cnl);
        }
#pragma unroll
        for (int v = 0; v < LOADS_K; ++v) {
            const long m = min(mbase + v * RPK + rowk, p.M - 1);
            rx[v] = *reinterpret_cast<const bf16x8*>(p.x + m * p.ldx + ckl);
        }
    };
    // the first chunk's loads leave before anything else: they are HBM-cold, and the W staging, the constants and the
    // two barriers of the prologue below used to stand in front of them in every workgroup
    const long stride = (long)gs.nbx * 4;
    long chunk = (long)gs.bx * 4 + wave;
    if (chunk < nchunks) fetch(chunk);

    // per-channel constants live in LDS (shared by the four waves) and are re-read at each stash: holding the
    // 9 x 8 floats per lane in registers costs a whole occupancy step
    float* cst = reinterpret_cast<float*>(ldsb + 4 * SLAB);       // [9][64]
    // W (N x K fp32, <= 16 KB) is staged through the still-unused slab area with coalesced loads (building the MFMA
    // fragments straight from global memory was 8 * NS * TK dependent scalar loads per lane).  It is staged as the
    // fragments want it: rounded to bf16 (the one rounding of each fp32 weight), transposed to [k][n] and zero-padded
    // to the TN*32 x TK*32 tile, so that a fragment is ONE unconditional 16-byte LDS read; the predicated form was
    // 8 * NS * TK single reads, each in an exec-mask region of its own.
    constexpr int WP = TN * 32 + 8;                               // row pitch (bf16): rows stay 16-byte aligned
    // WLDS (the recompute variant of the 2 x 2 tile): the recompute's W fragments would be 32 more registers on top of
    // wb's 32 and the 64 accumulators, i.e. scratch; there the staging lies behind the constants, in the part of the
    // allocation that only the fold at the end uses, stays for the whole kernel and the fragments are read per chunk
    constexpr bool WLDS = REC && TN * TK == 4;
    bf16_t* wl = reinterpret_cast<bf16_t*>(WLDS ? ldsb + 4 * SLAB + 9 * 64 * 4 : ldsb);
    float wv[TN * TK * 4];                                        // requested here, written to LDS after the constants:
#pragma unroll                                                    // both sets of loads are in flight together
    for (int it = 0; it < TN * TK * 4; ++it) {                    // clamped address, select after: loads back to back
        const int i = it * 256 + tid, n = i / (TK * 32), k = i % (TK * 32);
        wv[it] = p.w[min(n, p.N - 1) * p.K + min(k, p.K - 1)];
    }
    if (tid < 64) {
        const int cn = min(tid, p.N - 1), ck = min(tid, p.K - 1);
        cst[0 * 64 + tid] = p.ysc[cn]; cst[1 * 64 + tid] = p.ysh[cn]; cst[2 * 64 + tid] = p.ymu[cn];
        float r0 = 0.f, r1 = 0.f;                                             // fold the ISA_STAT_R replicas
#pragma unroll
        for (int r = 0; r < ISA_STAT_R; ++r) { r0 += p.yred[r * 2 * p.N + cn]; r1 += p.yred[r * 2 * p.N + p.N + cn]; }
        cst[3 * 64 + tid] = p.yis[cn] * (r1 * p.ycnt_inv);                    // invstd * mean(g' * yhat)
        cst[4 * 64 + tid] = r0 * p.ycnt_inv;                                  // mean(g')
        if (gs.bx == 0 && tid < p.N) {                                        // BN(y) parameter gradients (per group)
            if (p.ydgamma) atomicAdd(p.ydgamma + tid, r1);
            if (p.ydbeta) atomicAdd(p.ydbeta + tid, r0);
        }
        cst[5 * 64 + tid] = (XMODE && p.xsc) ? p.xsc[ck] : 1.f; cst[6 * 64 + tid] = (XMODE && p.xsh) ? p.xsh[ck] : 0.f;
        cst[7 * 64 + tid] = (XMODE && p.xmu) ? p.xmu[ck] : 0.f; cst[8 * 64 + tid] = (XMODE && p.xis) ? p.xis[ck] : 1.f;
    }
#pragma unroll
    for (int it = 0; it < TN * TK * 4; ++it) {
        const int i = it * 256 + tid, n = i / (TK * 32), k = i % (TK * 32);
        wl[k * WP + n] = (bf16_t)((n < p.N && k < p.K) ? wv[it] : 0.f);
    }
    __syncthreads();
    PHASE(1);
    auto ldc = [&](int which, int c0, float (&v)[8]) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(cst + which * 64 + c0), b = *reinterpret_cast<const f32x4*>(cst + which * 64 + c0 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
    };
    // ---- W fragments for the data gradient: B[n = 16 s + 8 hh + jj][k = 32 j + r]
    bf16x8 wb[NS][TK];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int j = 0; j < TK; ++j)
            wb[s][j] = *reinterpret_cast<const bf16x8*>(wl + (32 * j + r) * WP + 16 * s + 8 * hh);
    // ---- W fragments for the recompute of y: B[k = 32 g + 16 hh + 8 q + jj][n = 32 i + r], step 2 g + q.  The forward
    // kernel gives the upper half-wave the upper 16 channels of a 32-group (its A fragments are contiguous row pieces),
    // and an MFMA's result depends on which contraction slot a product sits in: the same assignment here
    constexpr bool WREG = REC && !WLDS;
    bf16x8 wf[WREG ? 2 * TK : 1][WREG ? TN : 1];
    if constexpr (WREG) {
#pragma unroll
        for (int s = 0; s < 2 * TK; ++s)
#pragma unroll
            for (int i = 0; i < TN; ++i) wf[s][i] = rec_wfrag<WP>(wl, s, i, lane);
    }
    __syncthreads();                                              // the slabs reuse W's staging area
    PHASE(2);

    f32x16 acc[TN][TK];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TK; ++j) acc[i][j] = f32x16{0};
    float s0[8], s1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s0[j] = 0.f; s1[j] = 0.f; }
    // bias gradient partials: channel 32 i + r, this half-wave's 16 pixels of every chunk (the accumulator layout)
    constexpr int NSB = BIAS ? TN : 1;
    float sb[NSB];
#pragma unroll
    for (int j = 0; j < NSB; ++j) sb[j] = 0.f;
    // the recompute's bias values, channel 32 i + r: loaded once, ahead of the loop.  (A load inside the loop is waited for
    // with the next chunk's prefetch in front of it in the in-order counter, i.e. it drains the prefetch.)
    float bvr[BIAS && REC ? TN : 1];
    if constexpr (BIAS && REC) {
#pragma unroll
        for (int i = 0; i < TN; ++i) bvr[i] = rec_bias<REC, BIAS>(p)[min(32 * i + r, p.N - 1)];
    }

    auto stash = [&](long chunk) {                               // BN-backward / prologue arithmetic, then LDS
        const long mbase = chunk * PMB;
        if constexpr (REC) {                                      // raw g; recompute() turns it into dy
#pragma unroll
            for (int v = 0; v < LOADS_N; ++v) *reinterpret_cast<bf16x8*>(sD + (v * RPN + rown) * SN + cgn * 16) = rg[v];
        } else {
        float ysc[8], ysh[8], ymu[8], yq[8], yk0[8];
        ldc(0, cn0, ysc); ldc(1, cn0, ysh); ldc(2, cn0, ymu); ldc(3, cn0, yq); ldc(4, cn0, yk0);
#pragma unroll
        for (int v = 0; v < LOADS_N; ++v) {
            const bool ok = (mbase + v * RPN + rown) < p.M && nok;
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float yy = (float)ry[v][j];
                const float dz = (float)rg[v][j] * act_grad_t<YACT>(fmaf(yy, ysc[j], ysh[j]), p.yact);
                const float val = ysc[j] * (dz - yk0[j] - (yy - ymu[j]) * yq[j]);
                o[j] = (bf16_t)((ok && cn0 + j < p.N) ? val : 0.f);
            }
            *reinterpret_cast<bf16x8*>(sD + (v * RPN + rown) * SN + cgn * 16) = o;
        }
        }
        float xsc[8], xsh[8];
        ldc(5, ck0, xsc); ldc(6, ck0, xsh);
#pragma unroll
        for (int v = 0; v < LOADS_K; ++v) {
            const bool ok = (mbase + v * RPK + rowk) < p.M && kok;
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xr = (float)rx[v][j];
                const float z = XMODE ? act_t<XACT>(fmaf(xr, xsc[j], xsh[j]), p.xact) : xr;
                o[j] = (bf16_t)((ok && ck0 + j < p.K) ? z : 0.f);
            }
            *reinterpret_cast<bf16x8*>(sX + (v * RPK + rowk) * SK + cgk * 16) = o;
            rxc[v] = rx[v];                                       // raw x of THIS chunk for the BN(x) sums
        }
    };

    for (; chunk < nchunks; chunk += stride) {
        stash(chunk);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        PHASE_ONCE(3);
        // operands of this chunk's store epilogue (old dx / residual-branch gradient): requested now, BEFORE the next
        // chunk's loads, and consumed after the MFMAs: their latency is not exposed at the end of the trip, and waiting
        // for them does not wait for the prefetch behind them
        constexpr bool EPI_PREFETCH = EPI && TK == 1;             // wider x tiles have no registers to spare
        bf16x8 repi_old[EPI_PREFETCH ? LOADS_K : 1], repi_add[EPI_PREFETCH ? LOADS_K : 1];
        if constexpr (EPI_PREFETCH) {
            const long mb = chunk * PMB;
#pragma unroll
            for (int v = 0; v < LOADS_K; ++v) {
                const long m = min(mb + v * RPK + rowk, p.M - 1);
                repi_old[v] = bf16x8{0}; repi_add[v] = bf16x8{0};
                if (p.accumulate) repi_old[v] = *reinterpret_cast<const bf16x8*>(p.dx + m * p.lddx + ckl);
                if (p.addend) repi_add[v] = *reinterpret_cast<const bf16x8*>(p.addend + m * p.lda + ckl);
            }
        }
        if (chunk + stride < nchunks) fetch(chunk + stride);
        if constexpr (REC) {
            // y tile of the chunk in the accumulator layout (lane = channel 32 i + r, 16 pixels), rounded as the forward
            // stored it, then dy over raw g in the dy slab: every lane reads and rewrites its own elements.  What lies past
            // M or N is zeroed by an AND on the stored bits: written as a select, the element's LDS read and arithmetic
            // were sunk into an exec-mask region of its own, 16 dependent LDS round trips per tile
            const int rows = (int)min((long)PMB, p.M - chunk * PMB) - 4 * hh;
#pragma unroll
            for (int i = 0; i < TN; ++i) {                        // one 32-channel tile at a time: 16 live accumulators
                f32x16 ya = f32x16{0};
#pragma unroll
                for (int s = 0; s < 2 * TK; ++s) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8*>(sX + r * SK + (32 * (s >> 1) + 16 * hh + 8 * (s & 1)) * 2);
                    bf16x8 b;
                    if constexpr (WLDS) b = rec_wfrag<WP>(wl, s, i, lane); else b = wf[s][i];
                    ya = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, ya, 0, 0, 0);
                }
                const int n = 32 * i + r;
                const float ysc = cst[0 * 64 + n], ysh = cst[1 * 64 + n], ymu = cst[2 * 64 + n], yq = cst[3 * 64 + n], yk0 = cst[4 * 64 + n];
                const unsigned colm = n < p.N ? 0xffffu : 0u;
                unsigned short* d = reinterpret_cast<unsigned short*>(sD + 4 * hh * SN + n * 2);
                unsigned short gr[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) gr[e] = d[((e & 3) + 8 * (e >> 2)) * (SN / 2)];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if constexpr (BIAS) {                         // y = W . pro(x) + bias, rounded as the forward's epilogue stored it
                        const float val = bn_bwd_dy<YACT>(__uint_as_float((unsigned)gr[e] << 16), (float)(bf16_t)(ya[e] + bvr[i]), ysc, ysh, ymu, yq, yk0, p.yact);
                        const unsigned o = __builtin_bit_cast(unsigned short, (bf16_t)val);
                        const unsigned om = o & ((e & 3) + 8 * (e >> 2) < rows ? colm : 0u);
                        d[((e & 3) + 8 * (e >> 2)) * (SN / 2)] = (unsigned short)om;
                        sb[i] += __uint_as_float(om << 16);
                    } else {
                    const float val = bn_bwd_dy<YACT>(__uint_as_float((unsigned)gr[e] << 16), (float)(bf16_t)ya[e], ysc, ysh, ymu, yq, yk0, p.yact);
                    const unsigned o = __builtin_bit_cast(unsigned short, (bf16_t)val);
                    d[((e & 3) + 8 * (e >> 2)) * (SN / 2)] = (unsigned short)(o & ((e & 3) + 8 * (e >> 2) < rows ? colm : 0u));
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else if constexpr (BIAS) {
#pragma unroll
            for (int i = 0; i < TN; ++i) {
                const unsigned short* d = reinterpret_cast<const unsigned short*>(sD + 4 * hh * SN + (32 * i + r) * 2);
                unsigned short dv[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) dv[e] = d[((e & 3) + 8 * (e >> 2)) * (SN / 2)];
#pragma unroll
                for (int e = 0; e < 16; ++e) sb[i] += __uint_as_float((unsigned)dv[e] << 16);
            }
        }
        // ---- weight gradient
#pragma unroll
        for (int s = 0; s < PMB / 16; ++s) {
            bf16x8 a[TN], b[TK];
#pragma unroll
            for (int i = 0; i < TN; ++i) a[i] = tr_frag(sD, SN, 16 * s, i * 32, lane);
#pragma unroll
            for (int j = 0; j < TK; ++j) b[j] = tr_frag(sX, SK, 16 * s, j * 32, lane);
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TK; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        // ---- data gradient for the 32 pixels of this chunk
        f32x16 dxa[TK];
#pragma unroll
        for (int j = 0; j < TK; ++j) dxa[j] = f32x16{0};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(sD + r * SN + (16 * s + 8 * hh) * 2);
#pragma unroll
            for (int j = 0; j < TK; ++j)
                dxa[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, wb[s][j], dxa[j], 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                          // all transpose reads of sX are done
#pragma unroll
        for (int j = 0; j < TK; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (e & 3) + 8 * (e >> 2) + 4 * hh;
                *reinterpret_cast<bf16_t*>(sX + row * SK + (32 * j + r) * 2) = (bf16_t)dxa[j][e];
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const long mbase = chunk * PMB;
        float xsc[8], xsh[8], xmu[8], xis[8];
        if (want_xred) { ldc(5, ck0, xsc); ldc(6, ck0, xsh); ldc(7, ck0, xmu); ldc(8, ck0, xis); }
#pragma unroll
        for (int v = 0; v < LOADS_K; ++v) {
            const long m = mbase + v * RPK + rowk;
            if (m < p.M && kok) {
                bf16x8 o = *reinterpret_cast<const bf16x8*>(sX + (v * RPK + rowk) * SK + cgk * 16);
                bf16_t* dst = p.dx + m * p.lddx + ck0;
                if constexpr (EPI) {
                    if (p.accumulate) {
                        bf16x8 old;
                        if constexpr (EPI_PREFETCH) old = repi_old[v]; else old = *reinterpret_cast<const bf16x8*>(dst);
#pragma unroll
                        for (int j = 0; j < 8; ++j) o[j] = (bf16_t)((float)o[j] + (float)old[j]);
                    }
                    if (p.addend) {
                        bf16x8 ad;
                        if constexpr (EPI_PREFETCH) ad = repi_add[v]; else ad = *reinterpret_cast<const bf16x8*>(p.addend + m * p.lda + ck0);
#pragma unroll
                        for (int j = 0; j < 8; ++j) o[j] = (bf16_t)((float)o[j] + (float)ad[j]);
                    }
                }
                *reinterpret_cast<bf16x8*>(dst) = o;
                if (want_xred) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float xr = (float)rxc[v][j];
                        const float dz = (float)o[j] * act_grad_t<XACT>(fmaf(xr, xsc[j], xsh[j]), p.xact);
                        s0[j] += dz; s1[j] += dz * ((xr - xmu[j]) * xis[j]);
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                          // sX is rewritten by the next stash
    }

    // ---- cross-wave fold (tr_lds.hpp): one slab per workgroup in the conv_wgrad.hip layout.  The BN(x) sums ride on
    // the same two barriers: every 16-lane row of every wave parks its row_fold partials in a slot of its own, and one
    // thread per channel adds the 16 slots in a fixed order - no same-address LDS atomics, no barriers of their own.
    PHASE(4);
    __syncthreads();                                              // the parked partials reuse the tile slabs and cst
    PHASE(5);
    float* part = reinterpret_cast<float*>(ldsb);
    float* xs = part + fold_part_floats<TN, TK>();                // [4 waves][4 rows][2][TK*32]
    fold_park<TN, TK>(part, acc, wave, lane);
    if (want_xred) {
        float* slot = xs + (wave * 4 + (lane >> 4)) * (2 * TK * 32);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v0 = row_fold<VK>(s0[j]), v1 = row_fold<VK>(s1[j]);      // lanes with equal lane % VK share channels
            if ((lane & 15) < VK) { slot[ck0 + j] = v0; slot[TK * 32 + ck0 + j] = v1; }
        }
    }
    // bias gradient: the two half-waves hold the same channels; every wave parks one slot
    float* bs = xs + 16 * 2 * TK * 32;                            // [4 waves][TN*32]
    if constexpr (BIAS) {
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const float v = sb[i] + __shfl_xor(sb[i], 32, 64);
            if (lane < 32) bs[wave * (TN * 32) + 32 * i + r] = v;
        }
    }
    __syncthreads();
    PHASE(6);
    constexpr int SLABF = TN * TK * 1024 + TN * 32;
    float* slab = p.ws + (long)blockIdx.x * SLABF;
    fold_store<TN, TK>(part, slab, tid);
    PHASE(7);
    if constexpr (BIAS) {
        if (tid < TN * 32) {                                      // column sums of dy: the fold adds them to dbias
            float v = 0.f;
#pragma unroll
            for (int sl = 0; sl < 4; ++sl) v += bs[sl * (TN * 32) + tid];
            slab[TN * TK * 1024 + tid] = v;
        }
    } else {
        if (tid < TN * 32) slab[TN * TK * 1024 + tid] = 0.f;     // no conv bias on this path
    }
    if (want_xred && tid < 2 * TK * 32) {
        float v = 0.f;
#pragma unroll
        for (int sl = 0; sl < 16; ++sl) v += xs[sl * (2 * TK * 32) + tid];
        const int which = tid / (TK * 32), c = tid - which * TK * 32;
        if (c < p.K && v != 0.f)
            atomicAdd(p.xred + (blockIdx.x & (ISA_STAT_R - 1)) * 2 * p.K + which * p.K + c, v);
    }
    PHASE(8);
    PHASE_FLUSH(phase_buf);
}

template <int TN, int TK, int YACT, int XMODE, bool REC, bool BIAS>
int launch_inst(PwParams& p, const float* bias, float* dbias, long ws_floats, isa_slab_arena* sa, const isa_pro* xfin, int xfin_groups, hipStream_t s) {
    constexpr int SN = TrStride<TN * 32>::bytes, SK = TrStride<TK * 32>::bytes;
    constexpr size_t slab = (size_t)32 * (SN + SK) * 4 + 9 * 64 * 4;
    constexpr size_t redb = ((size_t)fold_part_floats<TN, TK>() + 16 * 2 * TK * 32 + (BIAS ? 4 * TN * 32 : 0)) * 4;   // parked partials + BN(x) sum slots (+ bias slots)
    constexpr size_t wkeep = (REC && TN * TK == 4) ? (size_t)TK * 32 * (TN * 32 + 8) * 2 : 0;     // WLDS: W stays behind the constants
    constexpr size_t lds = slab + wkeep > redb ? slab + wkeep : redb;
    const long nchunks = (p.M + 31) / 32;
    long want = (nchunks + 3) / 4 * p.G, gx;
    if (want > 256 * 2) want = 256 * 2;                              // 2 resident workgroups per CU; fewer slabs to reduce
    if (int rc = slab_plan(sa, &p.ws, ws_floats, want, (long)TN * TK * 1024 + TN * 32, p.G, &gx)) return rc;
    if (int rc = fin_standalone(xfin, p.K, xfin_groups, s)) return rc;      // every check has passed
    constexpr int XM = XMODE | (BIAS ? PW_BIAS : 0);
    PwParams q = p;
    if constexpr (BIAS && REC) set_rec_bias<REC, BIAS>(q, bias);
    if (p.accumulate || p.addend) hipLaunchKernelGGL((pw_bn_bwd_kernel<TN, TK, YACT, XM, true, REC>), dim3((unsigned)gx), dim3(256), lds, s, q);
    else hipLaunchKernelGGL((pw_bn_bwd_kernel<TN, TK, YACT, XM, false, REC>), dim3((unsigned)gx), dim3(256), lds, s, q);
    if (launch_status() != ISA_OK) return ISA_ELAUNCH;
    return wgrad_slab_reduce_launch(p.ws, p.dw, BIAS ? dbias : nullptr, (int)gx, TN, TK, p.N, p.K, 1, sa, s);
}

template <int TN, int TK, bool BIAS>
int launch_tile(PwParams& p, const float* bias, float* dbias, int xmode, long ws_floats, isa_slab_arena* sa, const isa_pro* xfin, int xfin_groups, hipStream_t s) {
    // REC (y == NULL, recomputed): only the two compile-time activations have that form; the entry point refused the rest
    return by_int<ISA_ACT_RELU6, ISA_ACT_NONE, ACT_RT>(p.yact, [&](auto ya) { return by_int<0, 1, 2>(xmode, [&](auto xm) {
        auto go = [&](auto rec) {
            return launch_inst<TN, TK, decltype(ya)::value, decltype(xm)::value, decltype(rec)::value, BIAS>(
                p, bias, dbias, ws_floats, sa, xfin, xfin_groups, s);
        };
        if constexpr (decltype(ya)::value == ACT_RT) return go(std::false_type{});
        else return by_flag(!p.y, go);
    }); });
}

}  // namespace

#ifdef ISA_PHASE_TRACE
extern "C" int isa_phase_trace_pw(unsigned long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(phase_buf), sizeof(phase_buf)) == hipSuccess ? ISA_OK : ISA_ELAUNCH; }
#endif

// bias / dbias: both or neither (the conv's bias and its gradient); see include/isa_kernels.h
extern "C" int isa_conv1x1_bias_bn_backward(const isa_tensor* g, const isa_tensor* y, const isa_bn_bwd* ybn,
                                            const isa_tensor* x, const isa_pro* xpro, const isa_bn_bwd* xbn,
                                            const float* w, float* dw, const isa_tensor* dx, int32_t accumulate,
                                            const isa_tensor* addend, float* ws, int64_t ws_floats, isa_slab_arena* defer,
                                            void* stream, const float* bias, float* dbias) {
    if ((bias == nullptr) != (dbias == nullptr)) return ISA_EINVAL;
    if (!tensor_ok(g, 8) || (y && !tensor_ok(y, 8)) || !tensor_ok(x, 8) || !tensor_ok(dx, 8)) return ISA_EINVAL;
    if (!fin_valid(xpro)) return ISA_EINVAL;      // a pending finalize (no in-kernel form here) runs after the last check
    if (g->dtype != ISA_BF16 || (y && y->dtype != ISA_BF16) || x->dtype != ISA_BF16 || dx->dtype != ISA_BF16) return ISA_EINVAL;
    if (!bn_bwd_ok(ybn) || !xbn_ok(xbn)) return ISA_EINVAL;
    if (!w || !dw || (!ws && !defer)) return ISA_EINVAL;
    // y == NULL: recomputed in the kernel, which has that form for the two compile-time activations only
    if (!y && ybn->act != ISA_ACT_RELU6 && ybn->act != ISA_ACT_NONE) return ISA_EINVAL;
    const int N = g->c, K = x->c;
    if (N > 64 || K > 64 || N % 8 || K % 8) return ISA_EINVAL;
    if ((y && y->c != N) || dx->c != K) return ISA_EINVAL;
    const isa_tensor* ts[3] = {y, x, dx};
    for (const isa_tensor* t : ts)
        if (t && (t->n != g->n || t->h != g->h || t->w != g->w)) return ISA_EINVAL;
    const ProDev xp = make_pro(xpro);
    if (xp.bscale) return ISA_EINVAL;
    if (addend && !addend_ok(addend, g, K)) return ISA_EINVAL;
    PwParams p{};
    p.g = (const bf16_t*)g->data; p.y = y ? (const bf16_t*)y->data : nullptr; p.x = (const bf16_t*)x->data; p.dx = (bf16_t*)dx->data;
    p.w = w; p.dw = dw; p.N = N; p.K = K; p.ldg = g->ld; p.ldy = y ? y->ld : 0; p.ldx = x->ld; p.lddx = dx->ld;
    p.G = stat_groups(g, true);                                   // BN(y) constants and sums are per statistic group
    if (!p.G) return ISA_EINVAL;
    p.M = (long)(g->n / p.G) * g->h * g->w;
    set_bn_bwd(p, ybn, xp, xbn);
    p.accumulate = accumulate; p.ws = ws;
    if (addend) { p.addend = (const bf16_t*)addend->data; p.lda = addend->ld; }
    const int xmode = fused_xmode(xp, xbn);
    hipStream_t s = as_stream(stream);
    const int tn = (N + 31) / 32, tk = (K + 31) / 32;
    return by_flag(bias != nullptr, [&](auto b) { return by_int<1, 2>(tn, [&](auto n) { return by_int<1, 2>(tk, [&](auto k) {
        return launch_tile<decltype(n)::value, decltype(k)::value, decltype(b)::value>(p, bias, dbias, xmode, ws_floats, defer, xpro,
                                                                                        tensor_groups(x), s);
    }); }); });
}

extern "C" int isa_conv1x1_bn_backward(const isa_tensor* g, const isa_tensor* y, const isa_bn_bwd* ybn,
                                       const isa_tensor* x, const isa_pro* xpro, const isa_bn_bwd* xbn,
                                       const float* w, float* dw, const isa_tensor* dx, int32_t accumulate,
                                       const isa_tensor* addend, float* ws, int64_t ws_floats, isa_slab_arena* defer,
                                       void* stream) {
    return isa_conv1x1_bias_bn_backward(g, y, ybn, x, xpro, xbn, w, dw, dx, accumulate, addend, ws, ws_floats, defer, stream,
                                        nullptr, nullptr);
}
