// LDS transpose-read fragments for bf16 MFMA operands whose contraction index is the pixel.
// Tiles are staged row-major [pixel][channel]; ds_read_b64_tr_b16 returns, for lane (r, h), element j
// <- tile[8h+j][r] (verified by scripts/probes/tr_probe.hip).  Row stride == 64 (mod 256) bytes keeps the
// four 64-byte row pieces a half-wave touches on disjoint banks.
#pragma once
#include "common.hpp"

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
#define LDS_S16X4(ptr) ((__attribute__((address_space(3))) s16x4*)(ptr))

template <int CH> struct TrStride { static constexpr int bytes = (CH * 2) % 128 == 0 ? CH * 2 + 64 : CH * 2; };

// ---- phase trace (-DISA_PHASE_TRACE, off by default): wall_clock64() stamps (100 MHz) of thread 0 of workgroup 0 at the
// phase boundaries of one launch, kept in registers and written at the end with ordinary stores into a __device__ buffer
// of the translation unit; isa_phase_trace_pw / _wg copy it out (profiles/fixed_cost_phases.txt)
#ifdef ISA_PHASE_TRACE
#define PHASE_DECL() unsigned long long ph_[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define PHASE(i) (ph_[i] = wall_clock64())
#define PHASE_ONCE(i) do { if (ph_[i] == 0) ph_[i] = wall_clock64(); } while (0)
#define PHASE_FLUSH(buf) do { if (blockIdx.x + blockIdx.y + blockIdx.z == 0 && threadIdx.x == 0) { _Pragma("unroll") for (int i_ = 0; i_ < 10; ++i_) (buf)[i_] = ph_[i_]; } } while (0)
#else
#define PHASE_DECL() do {} while (0)
#define PHASE(i) do {} while (0)
#define PHASE_ONCE(i) do {} while (0)
#define PHASE_FLUSH(buf) do {} while (0)
#endif

// ---- cross-wave fold of the weight-gradient fragments of a 256-thread workgroup ---------------------------
// Every wave parks its TN x TK accumulator tiles (raw fragment layout: element e of lane l at [e * 64 + l]) in a
// region of its own, so the four parks run at once; after ONE barrier all 256 threads add the four partials of
// their elements in the order wave 0 + 1 + 2 + 3 (the order of the former serial fold: the slabs keep their bits)
// and store the slab with 1 KB coalesced rows.  The serial form was four barrier-separated phases in which one
// wave did TN*TK*16 LDS read-modify-writes while three waited, then 16-64 stores by wave 0 alone.
// LDS: fold_part_floats<TN, TK>() floats from `part`; the caller puts a __syncthreads() between its last use of
// that memory and fold_park, and one between fold_park and fold_store.  A wave without work parks its zeros.
template <int TN, int TK> constexpr int fold_part_floats() { return 4 * TN * TK * 1024; }
template <int TN, int TK>
__device__ __forceinline__ void fold_park(float* part, const f32x16 (&acc)[TN][TK], int wave, int lane) {
    float* mine = part + wave * (TN * TK * 1024) + lane;
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TK; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) mine[((i * TK + j) * 16 + e) * 64] = acc[i][j][e];
}
template <int TN, int TK>
__device__ __forceinline__ void fold_store(const float* part, float* slab, int tid) {
    constexpr int ACC = TN * TK * 1024;
#pragma unroll
    for (int i = 0; i < ACC / 256; ++i) {
        const float* q = part + i * 256 + tid;
        slab[i * 256 + tid] = 0.f + q[0] + q[ACC] + q[2 * ACC] + q[3 * ACC];
    }
}

__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int stride_bytes, int pix0, int chan0, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, pp = i & 3;
    const char* a = tile + (pix0 + 8 * (g >> 1) + q) * stride_bytes + (chan0 + 16 * (g & 1) + 4 * pp) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(a));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(a + 4 * stride_bytes));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}
