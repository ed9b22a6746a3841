// K-class semantic criterion of the trainer (reference: Model.__define_criterion and the CE / Dice branches of
// __minibatch, code/lib/model.py:102-133,255-269; losses/dice.py:10-85; torch.nn.CrossEntropyLoss(weight)).
// The shipped 2-class, unweighted, fg-only Multi criterion keeps its own kernels (isa_mask_loss_sums, isa_sem_loss,
// isa_mask_loss_grad); these serve every other (criterion, class_weights, optimize_bg, n_classes) combination.
//
// Per step, logits l [B,H,W,K] NHWC (bf16 | fp32, ld = rup(K, 8)), labels y uint8 [B,H,W], p = softmax_c(l), g = onehot(y):
//   sums   one streaming pass: per image and class  A = sum p*g,  S = sum p,  T = sum g;  batch  sum w_y*nll,  sum w_y
//   assemble (one workgroup): CE = sum w_y*nll / sum w_y;  D_bc = (2A+1)/(S+T+1);  dice = mean_b(1 - mean_{c in C} w'_c D_bc)
//            coef [3*B*K + 1] = { u_bc = -w'_c / (B|C|) (0 off C) | ce_scale = 1 / sum w_y | 2/den_bc | (2A_bc+1)/den_bc^2 }
//   grad   d l_k = ce_scale * w_y * (p_k - [k == y]) + p_k * (v_k - sum_j p_j v_j),  v_c = u_c * (2 g_c/den_c - (2A_c+1)/den_c^2)
// The settings live in a device buffer cfg[4 + K] = {use_ce, use_dice, optimize_bg, 0, w_0 .. w_{K-1}} (weights 1 when
// the caller gives none: CrossEntropyLoss() is the mean, and w' = |C| w / sum w = 1), so a captured hipGraph follows
// in-place changes of the weights and flags.  Labels >= K are a precondition violation, not checked here (the
// reference raises IndexError in numpy's collate).
#include "common.hpp"

namespace {


constexpr int CFG_HDR = 4;       // cfg[0] use_ce, cfg[1] use_dice, cfg[2] optimize_bg, cfg[3] unused; weights follow

// KT = K rounded up to a multiple of 8 (8, 16, 24 or 32): the class loops unroll, accumulators stay in registers.
// Channels c >= K of the row (the ld padding) read as -inf: probability 0, no contribution.
template <typename T, int KT>
__device__ __forceinline__ void load_row(const T* q, int K, float (&l)[KT]) {
#pragma unroll
    for (int j = 0; j < KT / 8; ++j) {
        float v[8];
        load8<T>(q + 8 * j, v);                           // the row holds ld >= KT elements: always in bounds
#pragma unroll
        for (int i = 0; i < 8; ++i) l[8 * j + i] = (8 * j + i < K) ? v[i] : -INFINITY;
    }
}

// softmax of one row in place; returns log-sum-exp
template <int KT>
__device__ __forceinline__ float softmax_row(float (&l)[KT], float (&p)[KT]) {
    float mx = l[0];
#pragma unroll
    for (int c = 1; c < KT; ++c) mx = fmaxf(mx, l[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < KT; ++c) { p[c] = expf(l[c] - mx); s += p[c]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < KT; ++c) p[c] *= inv;
    return mx + logf(s);
}

// sums[b][3K] = {A[K], S[K], T[K]}, sums[B*3K] = sum w_y*nll, sums[B*3K+1] = sum w_y (zeroed by the caller).
// Grid (x chunks, B): a workgroup walks pixels of ONE image, keeps 3K+2 partials per lane, reduces them across its
// four waves through LDS and issues one atomic per destination (Guideline 12).
// PW: the CE weight of pixel i is m_i * w_y with m = pixw [B,H,W]; without it pixw is never read.
template <typename T, int KT, bool PW>
__global__ __launch_bounds__(256) void sem_k_sums_kernel(View x, const uint8_t* labels, const float* cfg, const float* pixw,
                                                         float* sums) {
    __shared__ float sh[4][3 * KT + 2];
    __shared__ float sw[KT];                               // class weights: an LDS read per pixel, not a global one
    const int b = blockIdx.y, K = x.c;
    const long L = (long)x.h * x.w;
    if (threadIdx.x < KT) sw[threadIdx.x] = (int)threadIdx.x < K ? cfg[CFG_HDR + threadIdx.x] : 0.f;
    __syncthreads();
    float A[KT], S[KT], Tg[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) { A[c] = 0.f; S[c] = 0.f; Tg[c] = 0.f; }
    float ce = 0.f, ws = 0.f;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < L; p += (long)gridDim.x * 256) {
        float l[KT], pr[KT];
        load_row<T, KT>(reinterpret_cast<const T*>(x.data) + ((long)b * L + p) * x.ld, K, l);
        const int y = labels[(long)b * L + p];
        const float lse = softmax_row<KT>(l, pr);
        float ly = 0.f;
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            const bool hit = c == y;
            S[c] += pr[c];
            A[c] += hit ? pr[c] : 0.f;
            Tg[c] += hit ? 1.f : 0.f;
            ly = hit ? l[c] : ly;
        }
        float w = sw[min(y, KT - 1)];                    // (the clamp only keeps a bad label's read inside sw)
        if constexpr (PW) w *= pixw[(long)b * L + p];
        ce += w * (lse - ly);
        ws += w;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < KT; ++c) {
        const float a = wave_sum(A[c]), s = wave_sum(S[c]), t = wave_sum(Tg[c]);
        if (lane == 0) { sh[wave][c] = a; sh[wave][KT + c] = s; sh[wave][2 * KT + c] = t; }
    }
    ce = wave_sum(ce); ws = wave_sum(ws);
    if (lane == 0) { sh[wave][3 * KT] = ce; sh[wave][3 * KT + 1] = ws; }
    __syncthreads();
    const int i = threadIdx.x;
    if (i < 3 * KT + 2) {
        const float r = sh[0][i] + sh[1][i] + sh[2][i] + sh[3][i];
        if (i < 3 * KT) {
            const int kind = i / KT, c = i - kind * KT;
            if (c < K && r != 0.f) atomicAdd(sums + (long)b * 3 * K + kind * K + c, r);
        } else if (r != 0.f) {
            atomicAdd(sums + (long)x.n * 3 * K + (i - 3 * KT), r);
        }
    }
}

// One workgroup.  coef as in the file header; scal = {CE, Dice} (0 for a term the criterion lacks).
__global__ __launch_bounds__(1024) void sem_k_assemble_kernel(const float* sums, const float* cfg, int B, int K,
                                                              float* coef, float* scal) {
    __shared__ float red[16];
    __shared__ float wsum_c;
    const bool use_ce = cfg[0] != 0.f, use_dice = cfg[1] != 0.f, bg = cfg[2] != 0.f;
    const float* wc = cfg + CFG_HDR;
    const int c0 = bg ? 0 : 1, nc = K - c0;
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int c = c0; c < K; ++c) s += wc[c];
        wsum_c = s;
    }
    __syncthreads();
    const float wnorm = (float)nc / wsum_c;                          // w'_c = |C| w_c / sum_{C} w
    for (int i = threadIdx.x; i < B * K; i += blockDim.x) {
        const int b = i / K, c = i - b * K;
        float u = 0.f;
        if (use_dice && c >= c0) {
            const float* s = sums + (long)b * 3 * K;
            const float A = s[c], den = s[K + c] + s[2 * K + c] + 1.f;
            // D = (2A+1)/den, dD/dp_c(i) = 2g/den - (2A+1)/den^2;  loss = mean_b(1 - mean_C w' D)
            u = -(wc[c] * wnorm / ((float)B * nc));
            coef[i] = u;                                             // times (2g/den - (2A+1)/den^2): the grad kernel
            coef[(long)B * K + 1 + i] = 2.f / den;                   //   reads 2/den and (2A+1)/den^2 per (b, c)
            coef[(long)2 * B * K + 1 + i] = (2.f * A + 1.f) / (den * den);
        } else {
            coef[i] = 0.f;
            coef[(long)B * K + 1 + i] = 0.f;
            coef[(long)2 * B * K + 1 + i] = 0.f;
        }
    }
    // per image: 1 - mean_C w'_c D_bc
    float d = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float* s = sums + (long)b * 3 * K;
        float acc = 0.f;
        for (int c = c0; c < K; ++c) {
            const float den = s[K + c] + s[2 * K + c] + 1.f;
            acc += wc[c] * wnorm * (2.f * s[c] + 1.f) / den;
        }
        d += 1.f - acc / (float)nc;
    }
    d = wave_sum(d);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    if (lane == 0) red[wave] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < nw; ++w) t += red[w];
        const float wnll = sums[(long)B * 3 * K], wy = sums[(long)B * 3 * K + 1];
        coef[(long)B * K] = use_ce ? 1.f / wy : 0.f;
        scal[0] = use_ce ? wnll / wy : 0.f;
        scal[1] = use_dice ? t / (float)B : 0.f;
    }
}

// d l_k = ce_scale * w_y * (p_k - [k == y]) + p_k * (v_k - sum_j p_j v_j),  v_c = u_c * (2 g_c / den_c - (2A_c+1)/den_c^2)
__device__ float k_unit_weight = 1.f;     // what the unweighted entry's pixels read in place of pixw

// pixw (may be NULL): the CE term is scaled by m = pixw of the pixel.  The flag is a run-time one ON PURPOSE: as two template
// instantiations the compiler contracted the two bodies differently (the exponential's argument fused into an fma in one
// and not in the other, packed fmas in one only), and pixw = 1 then differed from the unweighted entry in the last bit.
// One body serves both entries, so unit weights give the unweighted entry's bits by construction: cw * 1.0f is cw.  And it
// is a stride, not a branch - a loop-invariant branch would be unswitched into two loop bodies, compiled apart again: the
// unweighted entry reads the one device word above at stride 0.
template <typename T, int KT>
__global__ __launch_bounds__(256) void sem_k_grad_kernel(View x, const uint8_t* labels, const float* cfg, const float* coef,
                                                         const float* pixw, View dx, int accumulate) {
    __shared__ float su[4][KT];
    const int b = blockIdx.y, K = x.c, B = x.n;
    const long L = (long)x.h * x.w;
    if (threadIdx.x < KT) {
        const int c = threadIdx.x;
        const long i = (long)b * K + c;
        su[3][c] = c < K ? cfg[CFG_HDR + c] : 0.f;
        su[0][c] = c < K ? coef[i] : 0.f;
        su[1][c] = c < K ? coef[(long)B * K + 1 + i] : 0.f;
        su[2][c] = c < K ? coef[(long)2 * B * K + 1 + i] : 0.f;
    }
    __syncthreads();
    float u[KT], e2[KT], base[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) { u[c] = su[0][c]; e2[c] = su[1][c]; base[c] = -u[c] * su[2][c]; }
    const float ce_scale = coef[(long)B * K];
    const float* pw = pixw ? pixw + (long)b * L : &k_unit_weight;
    const long pw_stride = pixw ? 1 : 0;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < L; p += (long)gridDim.x * 256) {
        float l[KT], pr[KT];
        load_row<T, KT>(reinterpret_cast<const T*>(x.data) + ((long)b * L + p) * x.ld, K, l);
        const int y = labels[(long)b * L + p];
        softmax_row<KT>(l, pr);
        // v_c = base_c + [c == y] u_c * 2/den_c
        float sv = 0.f;
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            const float v = base[c] + (c == y ? u[c] * e2[c] : 0.f);
            l[c] = v;                                                 // reuse l[] for v
            sv += pr[c] * v;
        }
        const float cw = ce_scale * su[3][min(y, KT - 1)] * pw[p * pw_stride];
        T* d = reinterpret_cast<T*>(dx.data) + ((long)b * L + p) * dx.ld;
#pragma unroll
        for (int j = 0; j < KT / 8; ++j) {
            const int nv = K - 8 * j;
            if (nv <= 0) break;
            float o[8], old[8];
            if (accumulate) load8g<T>(d + 8 * j, old, nv);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = 8 * j + i;
                o[i] = cw * (pr[c] - (c == y ? 1.f : 0.f)) + pr[c] * (l[c] - sv);
                if (accumulate) o[i] += old[i];
            }
            store8g<T>(d + 8 * j, o, nv);
        }
    }
}

// logits: 2 <= K <= 32 classes, ld a multiple of 8 and 16-byte aligned rows (the vector loads read whole 8-groups)
static inline bool logits_ok(const isa_tensor* x) {
    return tensor_ok(x, 8) && x->c >= 2 && x->c <= ISA_SEM_MAX_CLASSES && tensor_groups(x) == 1;
}

}  // namespace

namespace {
template <bool PW>
int sem_k_sums(const isa_tensor* logits, const uint8_t* labels, const float* cfg, const float* pixw, float* sums,
               void* stream) {
    if (!logits_ok(logits) || !labels || !cfg || !sums || (PW && !pixw)) return ISA_EINVAL;
    if (PW && !aligned(pixw, 4)) return ISA_EALIGN;
    const long L = (long)logits->h * logits->w;
    dim3 grid(grid_cap(cdiv(L, 256), 64), logits->n);
    by_dtype(logits->dtype, [&](auto t) { by_width8(logits->c, [&](auto kt) {
        hipLaunchKernelGGL((sem_k_sums_kernel<decltype(t), decltype(kt)::value, PW>), grid, dim3(256), 0, as_stream(stream),
                           mkview(logits), labels, cfg, pixw, sums);
    }); });
    return launch_status();
}

template <bool PW>
int sem_k_grad(const isa_tensor* logits, const uint8_t* labels, const float* cfg, const float* coef, const float* pixw,
               const isa_tensor* dlogits, int32_t accumulate, void* stream) {
    if (!logits_ok(logits) || !tensor_ok(dlogits, 8) || !labels || !cfg || !coef || (PW && !pixw)) return ISA_EINVAL;
    if (!same_shape(dlogits, logits)) return ISA_EINVAL;
    if (PW && !aligned(pixw, 4)) return ISA_EALIGN;
    const long L = (long)logits->h * logits->w;
    dim3 grid(grid_cap(cdiv(L, 256), 128), logits->n);
    by_dtype(logits->dtype, [&](auto t) { by_width8(logits->c, [&](auto kt) {
        hipLaunchKernelGGL((sem_k_grad_kernel<decltype(t), decltype(kt)::value>), grid, dim3(256), 0, as_stream(stream),
                           mkview(logits), labels, cfg, coef, pixw, mkview(dlogits), accumulate);
    }); });
    return launch_status();
}
}  // namespace

extern "C" int isa_sem_loss_k_sums(const isa_tensor* logits, const uint8_t* labels, const float* cfg, float* sums,
                                   void* stream) {
    return sem_k_sums<false>(logits, labels, cfg, nullptr, sums, stream);
}

extern "C" int isa_sem_loss_k_sums_pw(const isa_tensor* logits, const uint8_t* labels, const float* cfg, const float* pixw,
                                      float* sums, void* stream) {
    return sem_k_sums<true>(logits, labels, cfg, pixw, sums, stream);
}

extern "C" int isa_sem_loss_k_assemble(const float* sums, const float* cfg, int32_t B, int32_t K, float* coef, float* scal,
                                       void* stream) {
    if (!sums || !cfg || !coef || !scal || B <= 0 || K < 2 || K > ISA_SEM_MAX_CLASSES) return ISA_EINVAL;
    hipLaunchKernelGGL(sem_k_assemble_kernel, dim3(1), dim3(1024), 0, as_stream(stream), sums, cfg, B, K, coef, scal);
    return launch_status();
}

extern "C" int isa_sem_loss_k_grad(const isa_tensor* logits, const uint8_t* labels, const float* cfg, const float* coef,
                                   const isa_tensor* dlogits, int32_t accumulate, void* stream) {
    return sem_k_grad<false>(logits, labels, cfg, coef, nullptr, dlogits, accumulate, stream);
}

extern "C" int isa_sem_loss_k_grad_pw(const isa_tensor* logits, const uint8_t* labels, const float* cfg, const float* coef,
                                      const float* pixw, const isa_tensor* dlogits, int32_t accumulate, void* stream) {
    return sem_k_grad<true>(logits, labels, cfg, coef, pixw, dlogits, accumulate, stream);
}

// ---- reference-format targets: int64 one-hot [B,K,H,W] -> uint8 labels [B,H,W] and the fp32 argmax map ----------------
namespace {
__global__ __launch_bounds__(256) void labels_from_onehot_kernel(const int64_t* oh, int K, long hw, long total,
                                                                 uint8_t* labels, float* amap) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / hw, p = i - b * hw;
        const int64_t* q = oh + b * K * hw + p;
        int64_t best = q[0];
        int arg = 0;
        for (int c = 1; c < K; ++c) {
            const int64_t v = q[(long)c * hw];
            if (v > best) { best = v; arg = c; }                     // first maximum wins (torch.argmax)
        }
        if (labels) labels[i] = (uint8_t)arg;
        if (amap) amap[i] = (float)arg;
    }
}
}  // namespace

extern "C" int isa_labels_from_onehot(const int64_t* onehot, int32_t n, int32_t k, int64_t hw, uint8_t* labels,
                                      float* argmax_map, void* stream) {
    if (!onehot || n <= 0 || k < 2 || k > 256 || hw <= 0 || (!labels && !argmax_map)) return ISA_EINVAL;
    const long total = (long)n * hw;
    hipLaunchKernelGGL(labels_from_onehot_kernel, dim3(grid_cap(cdiv(total, 256))), dim3(256), 0, as_stream(stream),
                       onehot, (int)k, (long)hw, total, labels, argmax_map);
    return launch_status();
}
