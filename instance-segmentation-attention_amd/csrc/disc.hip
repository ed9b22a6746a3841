// Discriminative embedding loss (reference: calculate_means / calculate_variance_term / calculate_distance_term /
// calculate_regularization_term / calculate_q_regularization_term / discriminative_loss,
// code/lib/losses/discriminative.py:7-62, 65-95, 98-132, 135-147, 149-160, 162-188) and its hand-derived backward.
//
// emb x [B,H,W,C] NHWC (bf16 | fp32, C <= 32, ld a multiple of 8), labels l uint8 [B, L = H*W] (0 background, i + 1 =
// instance i; labels above k count as background), n_b = n_objects[b] clamped to [0, 32].  Instance i of image b is
// PRESENT when i < n_b and N_i > 0; np_b = present instances, F_b = sum of their N_i.  |.| is the L1 or L2 norm (`norm`).
//   m_i = sum_{p in i} x_p / N_i,  mu_i = unit_means ? m_i / |m_i|_2 (0 when m_i = 0) : m_i       (absent: 0)
//   var  = 1/B sum_b 1/F_b sum_{i present} sum_{p in i} h_p^2,   h_p = max(|x_p - mu_i| - delta_v, 0)
//   dist = 1/B sum_{b: np_b >= 2} sum_{i != j present} max(2 delta_d - |mu_i - mu_j|, 0)^2 / (np_b (np_b - 1))
//   reg  = 1/B sum_{b: np_b >= 1} 1/np_b sum_{i present} |mu_i|
//   qreg = sum_{b,p} ([l_p != 0] |x_p|_2 - 1)^2 / num,  num = foreground pixels of the batch (every plane, counted or not)
//   loss = weight (alpha var + beta dist + gamma reg + gamma_q qreg)
// d|d|/dd is d/|d|_2 (0 at d = 0) or sign(d) (sign(0) = 0).  F_b = 0 / np_b < 2 / np_b = 0 / num = 0: the term is 0.
//   sums      one-hot[32 x P] . x[P x 32] on the f32-input MFMA (32x32x2: exact f32, a fixed fmaf chain): a wave stages 64
//             pixels in LDS (16-byte loads) and issues 32 MFMAs; a workgroup owns one chunk of a row and writes its own slab
//   means     one workgroup per image folds the chunk slabs in chunk order: mu, m, |m|_2, the integer counts
//   hinge     second pass: h_p d|d|/dd staged in LDS and summed per instance by the same MFMA; sum h^2 and the qreg summand
//             per chunk in double
//   assemble  per image: fold the hinge slabs, distance and regulariser terms over the <= 32 means, d loss / d mu, back through
//             the normalisation, gconst = weight g_m / N_i; then one workgroup folds the images in order: scal[8]
//   grad      third pass: dx_p = coef_b h_p d|d|/dd + gconst[l_p] + qcoef (|x_p| - 1) x_p / |x_p|, recomputed from x, mu, l
// cfg (device, read at run time: a captured hipGraph follows in-place changes) = {delta_v, delta_d, norm (informative: the
// kernels take the call argument), unit_means, alpha, beta, gamma, gamma_q, weight}.  No float atomics anywhere: every sum
// has a fixed order, loss and gradient are bit-reproducible.
#include "common.hpp"

namespace {

constexpr int NT = 256, NW = 4, TP = 64, KI = ISA_DISC_MAX_K, CH = 32, SLAB = KI * CH;
constexpr int CNT = ISA_DISC_CNT_STRIDE;


struct Geo { int chunks; long per; };
static inline Geo geometry(long L) {
    const int ch = (int)ISA_DISC_CHUNKS(L);
    return Geo{ch, ((L + ch - 1) / ch + TP - 1) / TP * TP};
}

// sum over the 4 lanes of a pixel (its channel groups): every lane of the quad ends with the same bits
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    return v;
}
// sum over the 32 lanes that share an instance row
__device__ __forceinline__ float row32_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ int clamp_nb(int v) { return v < 0 ? 0 : (v > KI ? KI : v); }

// 8 channels [8g, 8g+8) of pixel p of image b; channels >= c and groups past the last read as 0
template <typename T>
__device__ __forceinline__ void load_group(const View& x, long row, int g, float (&v)[8]) {
    const int nv = x.c - 8 * g;
    if (nv > 0) {
        const raw8<T> r = load8raw<T>(reinterpret_cast<const T*>(x.data) + row * x.ld + 8 * g);   // ld % 8 == 0: in the row
        unpack8m<T>(r, v, nv);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0.f;
    }
}
__device__ __forceinline__ void put_group(float* dst, const float (&v)[8]) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
}

// acc[i][j] += sum over the tile's 64 pixels of [lab == i + 1] * xs[pixel][j].  Lane l feeds A[i = l & 31][k = l >> 5] and
// B[k][j = l & 31]; D has j on the lane and i = (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r.
__device__ __forceinline__ void onehot_mma(const float (*xs)[CH], const int* labs, int lane, f32x16& acc) {
    const int half = lane >> 5, col = lane & 31;
#pragma unroll 8
    for (int s = 0; s < TP / 2; ++s) {
        const int px = 2 * s + half;
        const float a = labs[px] == col + 1 ? 1.f : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xs[px][col], acc, 0, 0, 0);
    }
}

// the four waves' accumulators -> out[SLAB] in wave order.  red: >= NW * SLAB floats of LDS nobody reads any more.
__device__ __forceinline__ void fold_acc(const f32x16& acc, float* red, float* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        red[wave * SLAB + i * CH + (lane & 31)] = acc[r];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SLAB; e += NT) out[e] = ((red[e] + red[SLAB + e]) + red[2 * SLAB + e]) + red[3 * SLAB + e];
}

// grid (chunks, B).  slab [B][chunks][32][32], cslab [B][chunks][32]
template <typename T>
__global__ __launch_bounds__(NT) void disc_sums_kernel(View x, const uint8_t* __restrict__ labels, int k, long per,
                                                       float* __restrict__ slab, int32_t* __restrict__ cslab) {
    __shared__ __attribute__((aligned(16))) float xs[NW][TP][CH];
    __shared__ int labs[NW][TP];
    __shared__ int cnt[KI];
    const int b = blockIdx.y, chunk = blockIdx.x, nch = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long L = (long)x.h * x.w, p0 = (long)chunk * per, p1 = p0 + per < L ? p0 + per : L;
    if (threadIdx.x < KI) cnt[threadIdx.x] = 0;
    f32x16 acc = {};
    const int rounds = (int)((per + NW * TP - 1) / (NW * TP));
    for (int r = 0; r < rounds; ++r) {
        const long base = p0 + ((long)r * NW + wave) * TP;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int item = q * 64 + lane, px = item >> 2, g = item & 3;
            float v[8];
            if (base + px < p1) load_group<T>(x, (long)b * L + base + px, g, v);
            else {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = 0.f;
            }
            put_group(&xs[wave][px][8 * g], v);
        }
        int lab = base + lane < p1 ? labels[(long)b * L + base + lane] : 0;
        if (lab > k) lab = 0;
        labs[wave][lane] = lab;
        if (lab) atomicAdd(&cnt[lab - 1], 1);
        __syncthreads();
        onehot_mma(xs[wave], labs[wave], lane, acc);
    }
    __syncthreads();
    const long o = (long)b * nch + chunk;
    if (threadIdx.x < KI) cslab[o * KI + threadIdx.x] = cnt[threadIdx.x];
    fold_acc(acc, &xs[0][0][0], slab + o * SLAB);
}

// grid B, 1024 threads: thread (i, j)
__global__ __launch_bounds__(1024) void disc_means_kernel(const float* __restrict__ slab, const int32_t* __restrict__ cslab,
                                                          const int32_t* __restrict__ nobj, const float* __restrict__ cfg,
                                                          int nch, float* __restrict__ mu, float* __restrict__ m,
                                                          float* __restrict__ mnorm, int32_t* __restrict__ cnt) {
    __shared__ int sN[KI], sP[KI];
    const int b = blockIdx.x, t = threadIdx.x, i = t >> 5, j = t & 31;
    const bool unit = cfg[3] != 0.f;
    const int nb = clamp_nb(nobj[b]);
    float s = 0.f;
    int N = 0;
    for (int ch = 0; ch < nch; ++ch) {
        s += slab[((long)b * nch + ch) * SLAB + t];
        N += cslab[((long)b * nch + ch) * KI + i];
    }
    const bool present = i < nb && N > 0;
    const float mv = present ? s / (float)N : 0.f;
    const float nrm = sqrtf(row32_sum(mv * mv));
    const float muv = unit ? (nrm > 0.f ? mv / nrm : 0.f) : mv;
    mu[(long)b * SLAB + t] = muv;
    if (m) m[(long)b * SLAB + t] = mv;
    if (j == 0) {
        mnorm[b * KI + i] = nrm;
        cnt[b * CNT + i] = N;
        sN[i] = N;
        sP[i] = present;
    }
    __syncthreads();
    if (t == 0) {
        int F = 0, np = 0, all = 0;
        for (int q = 0; q < KI; ++q) { all += sN[q]; if (sP[q]) { F += sN[q]; ++np; } }
        cnt[b * CNT + 32] = F;
        cnt[b * CNT + 33] = np;
        cnt[b * CNT + 34] = all;
        cnt[b * CNT + 35] = 0;
    }
}

// d = x - mu over the 8 channels of a lane, the pixel's norm over its quad; v = h d|d|/dd.  Returns h.
template <int NORM>
__device__ __forceinline__ float hinge_vec(const float (&x)[8], const float* mrow, bool active, float dv, float (&v)[8]) {
    float d[8], s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        d[i] = active ? x[i] - mrow[i] : 0.f;
        s += NORM == 2 ? d[i] * d[i] : fabsf(d[i]);
    }
    s = quad_sum(s);
    const float nd = NORM == 2 ? sqrtf(s) : s;
    const float h = active ? fmaxf(nd - dv, 0.f) : 0.f;
    const float f = NORM == 2 ? (nd > 0.f ? h / nd : 0.f) : h;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = NORM == 2 ? f * d[i] : f * sgn(d[i]);
    return h;
}

// grid (chunks, B).  hslab [B][chunks][32][32], partial [B][chunks][2] = {sum h^2, sum ([l != 0] |x|_2 - 1)^2}
template <typename T, int NORM>
__global__ __launch_bounds__(NT) void disc_hinge_kernel(View x, const uint8_t* __restrict__ labels, int k,
                                                        const int32_t* __restrict__ nobj, const float* __restrict__ mu,
                                                        const float* __restrict__ cfg, long per, float* __restrict__ hslab,
                                                        double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float xs[NW][TP][CH];
    __shared__ __attribute__((aligned(16))) float mus[KI][CH];
    __shared__ int labs[NW][TP];
    __shared__ double dred[NW][2];
    const int b = blockIdx.y, chunk = blockIdx.x, nch = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long L = (long)x.h * x.w, p0 = (long)chunk * per, p1 = p0 + per < L ? p0 + per : L;
    const int nb = clamp_nb(nobj[b]);
    const float dv = cfg[0];
    for (int e = threadIdx.x; e < SLAB; e += NT) (&mus[0][0])[e] = mu[(long)b * SLAB + e];
    f32x16 acc = {};
    double hs = 0.0, qs = 0.0;
    const int rounds = (int)((per + NW * TP - 1) / (NW * TP));
    for (int r = 0; r < rounds; ++r) {
        const long base = p0 + ((long)r * NW + wave) * TP;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int item = q * 64 + lane, px = item >> 2, g = item & 3;
            const bool valid = base + px < p1;
            float xv[8], v[8];
            int lab = 0;
            if (valid) {
                load_group<T>(x, (long)b * L + base + px, g, xv);
                lab = labels[(long)b * L + base + px];
                if (lab > k) lab = 0;
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) xv[i] = 0.f;
            }
            const bool active = lab >= 1 && lab <= nb;
            float sx = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) sx += xv[i] * xv[i];
            sx = quad_sum(sx);
            const float h = hinge_vec<NORM>(xv, &mus[active ? lab - 1 : 0][8 * g], active, dv, v);
            put_group(&xs[wave][px][8 * g], v);
            if (g == 0) {
                labs[wave][px] = active ? lab : 0;
                if (valid) {
                    const float qn = (lab ? sqrtf(sx) : 0.f) - 1.f;
                    hs += (double)h * (double)h;
                    qs += (double)qn * (double)qn;
                }
            }
        }
        __syncthreads();
        onehot_mma(xs[wave], labs[wave], lane, acc);
    }
    hs = wave_sum(hs);
    qs = wave_sum(qs);
    if (lane == 0) { dred[wave][0] = hs; dred[wave][1] = qs; }
    __syncthreads();
    const long o = (long)b * nch + chunk;
    if (threadIdx.x < 2) partial[o * 2 + threadIdx.x] = ((dred[0][threadIdx.x] + dred[1][threadIdx.x]) + dred[2][threadIdx.x]) + dred[3][threadIdx.x];
    fold_acc(acc, &xs[0][0][0], hslab + o * SLAB);
}

// grid B, 1024 threads: thread (i, j).  img [B][8] = {var_b, dist_b, reg_b, qreg sum, np_b, F_b, foreground, 0}
template <int NORM>
__global__ __launch_bounds__(1024) void disc_image_kernel(const float* __restrict__ hslab, const double* __restrict__ partial,
                                                          const float* __restrict__ mu, const float* __restrict__ mnorm,
                                                          const int32_t* __restrict__ cnt, const int32_t* __restrict__ nobj,
                                                          const float* __restrict__ cfg, int B, int nch,
                                                          float* __restrict__ gconst, float* __restrict__ coef,
                                                          double* __restrict__ img) {
    __shared__ float smu[KI][CH + 1], T[KI][KI + 1];
    __shared__ int sPres[KI];
    __shared__ double sh[16];
    const int b = blockIdx.x, t = threadIdx.x, i = t >> 5, j = t & 31;
    const float dd = cfg[1], alpha = cfg[4], beta = cfg[5], gamma = cfg[6], weight = cfg[8];
    const bool unit = cfg[3] != 0.f;
    const int nb = clamp_nb(nobj[b]);
    const int Ni = cnt[b * CNT + i], F = cnt[b * CNT + 32], np = cnt[b * CNT + 33];
    const bool present = i < nb && Ni > 0;
    float S = 0.f;
    for (int ch = 0; ch < nch; ++ch) S += hslab[((long)b * nch + ch) * SLAB + t];
    const float muv = mu[(long)b * SLAB + t];
    smu[i][j] = muv;
    if (j == 0) sPres[i] = present;
    __syncthreads();
    // pair (i, j)
    float ds = 0.f;
#pragma unroll 8
    for (int c = 0; c < CH; ++c) {
        const float df = smu[i][c] - smu[j][c];
        ds += NORM == 2 ? df * df : fabsf(df);
    }
    const float dist = NORM == 2 ? sqrtf(ds) : ds;
    const bool pair = present && sPres[j] && i != j && np >= 2;
    const float tt = pair ? fmaxf(2.f * dd - dist, 0.f) : 0.f;
    T[i][j] = NORM == 2 ? (dist > 0.f ? tt / dist : 0.f) : tt;
    const double pairs = np >= 2 ? (double)np * (double)(np - 1) : 1.0;
    const double dist_b = block_sum((double)tt * (double)tt, sh) / pairs;       // (its barriers publish T)
    // element (i, c = j)
    float gd = 0.f;
#pragma unroll 8
    for (int q = 0; q < KI; ++q) {
        const float df = muv - smu[q][j];
        gd += T[i][q] * (NORM == 2 ? df : sgn(df));
    }
    const float invB = 1.f / (float)B;
    const float rn = NORM == 2 ? sqrtf(row32_sum(muv * muv)) : row32_sum(fabsf(muv));
    const double reg_b = block_sum(present && j == 0 ? (double)rn : 0.0, sh) / (np > 0 ? (double)np : 1.0);
    float g = 0.f;
    if (present) {
        if (F > 0) g -= 2.f * alpha * invB / (float)F * S;
        if (np >= 2) g -= 4.f * beta * invB / (float)pairs * gd;
        g += gamma * invB / (float)np * (NORM == 2 ? (rn > 0.f ? muv / rn : 0.f) : sgn(muv));
    }
    if (unit) {
        const float dot = row32_sum(muv * g), mn = mnorm[b * KI + i];
        g = mn > 0.f ? (g - muv * dot) / mn : 0.f;
    }
    gconst[(long)b * SLAB + t] = present ? weight * g / (float)Ni : 0.f;
    if (t == 0) {
        double hs = 0.0, qs = 0.0;
        for (int ch = 0; ch < nch; ++ch) { hs += partial[((long)b * nch + ch) * 2]; qs += partial[((long)b * nch + ch) * 2 + 1]; }
        coef[b] = F > 0 ? weight * 2.f * alpha * invB / (float)F : 0.f;
        double* o = img + (long)b * 8;
        o[0] = F > 0 ? hs / (double)F : 0.0;
        o[1] = dist_b;
        o[2] = reg_b;
        o[3] = qs;
        o[4] = (double)np;
        o[5] = (double)F;
        o[6] = (double)cnt[b * CNT + 34];
        o[7] = 0.0;
    }
}

// one wave: lanes stride the images, fixed fold
__global__ __launch_bounds__(64) void disc_total_kernel(const double* __restrict__ img, const float* __restrict__ cfg, int B,
                                                        float* __restrict__ coef, float* __restrict__ scal) {
    double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < B; b += 64)
#pragma unroll
        for (int q = 0; q < 7; ++q) a[q] += img[(long)b * 8 + q];
#pragma unroll
    for (int q = 0; q < 7; ++q) a[q] = wave_sum(a[q]);
    if (threadIdx.x == 0) {
        const double var = a[0] / B, dist = a[1] / B, reg = a[2] / B, num = a[6];
        const double qreg = num > 0.0 ? a[3] / num : 0.0;
        const double loss = (double)cfg[4] * var + (double)cfg[5] * dist + (double)cfg[6] * reg + (double)cfg[7] * qreg;
        scal[0] = (float)((double)cfg[8] * loss);
        scal[1] = (float)var;
        scal[2] = (float)dist;
        scal[3] = (float)reg;
        scal[4] = (float)qreg;
        scal[5] = (float)a[4];
        scal[6] = (float)a[5];
        scal[7] = 0.f;
        coef[B] = num > 0.0 ? (float)((double)cfg[8] * 2.0 * (double)cfg[7] / num) : 0.f;
    }
}

// grid (x, B): item = (pixel, channel group of 8), four items per pixel
template <typename T, int NORM>
__global__ __launch_bounds__(NT) void disc_grad_kernel(View x, const uint8_t* __restrict__ labels, int k,
                                                       const int32_t* __restrict__ nobj, const float* __restrict__ mu,
                                                       const float* __restrict__ gconst, const float* __restrict__ coef,
                                                       const float* __restrict__ cfg, View dx, int accumulate) {
    __shared__ __attribute__((aligned(16))) float mus[KI][CH], gcs[KI][CH];
    const int b = blockIdx.y;
    const long L = (long)x.h * x.w;
    const int nb = clamp_nb(nobj[b]);
    const float dv = cfg[0], cv = coef[b], cq = coef[x.n];
    for (int e = threadIdx.x; e < SLAB; e += NT) {
        (&mus[0][0])[e] = mu[(long)b * SLAB + e];
        (&gcs[0][0])[e] = gconst[(long)b * SLAB + e];
    }
    __syncthreads();
    for (long it = (long)blockIdx.x * NT + threadIdx.x; it < 4 * L; it += (long)gridDim.x * NT) {
        const long p = it >> 2;
        const int g = (int)(it & 3);
        float xv[8], v[8];
        load_group<T>(x, (long)b * L + p, g, xv);
        int lab = labels[(long)b * L + p];
        if (lab > k) lab = 0;
        const bool active = lab >= 1 && lab <= nb;
        float sx = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) sx += xv[i] * xv[i];
        sx = quad_sum(sx);
        hinge_vec<NORM>(xv, &mus[active ? lab - 1 : 0][8 * g], active, dv, v);
        const float xn = sqrtf(sx);
        const float fq = (lab && xn > 0.f) ? cq * (xn - 1.f) / xn : 0.f;
        const float* gc = &gcs[lab ? lab - 1 : 0][8 * g];
        const int nv = x.c - 8 * g;
        if (nv <= 0) continue;
        T* d = reinterpret_cast<T*>(dx.data) + ((long)b * L + p) * dx.ld + 8 * g;
        float o[8], old[8];
        if (accumulate) load8g<T>(d, old, nv);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            o[i] = cv * v[i] + (lab ? gc[i] : 0.f) + fq * xv[i];
            if (accumulate) o[i] += old[i];
        }
        store8g<T>(d, o, nv);
    }
}

bool batch_ok(int32_t n, int64_t L) { return n >= 1 && n <= 65535 && L >= 1 && L < (1ll << 31); }

}  // namespace

extern "C" int isa_disc_sums(const isa_tensor* emb, const uint8_t* labels, int32_t k, float* slab, int32_t* cslab,
                             void* stream) {
    const int rc = emb_status(emb, CH);
    if (rc != ISA_OK) return rc;
    if (!labels || !slab || !cslab || k < 1 || k > KI) return ISA_EINVAL;
    if (!aligned(slab, 16) || !aligned(cslab, 4)) return ISA_EALIGN;
    const Geo geo = geometry((long)emb->h * emb->w);
    const dim3 grid(geo.chunks, emb->n);
    by_dtype(emb->dtype, [&](auto t) {
        hipLaunchKernelGGL(disc_sums_kernel<decltype(t)>, grid, dim3(NT), 0, as_stream(stream), mkview(emb), labels, (int)k, geo.per, slab, cslab);
    });
    return launch_status();
}

extern "C" int isa_disc_means(const float* slab, const int32_t* cslab, const int32_t* n_objects, const float* cfg, int32_t n,
                              int64_t L, float* mu, float* m, float* mnorm, int32_t* cnt, void* stream) {
    if (!slab || !cslab || !n_objects || !cfg || !mu || !mnorm || !cnt || !batch_ok(n, L)) return ISA_EINVAL;
    if (!aligned(slab, 16) || !aligned(cslab, 4) || !aligned(n_objects, 4) || !aligned(cfg, 4) || !aligned(mu, 16) ||
        !aligned(m, 16) || !aligned(mnorm, 4) || !aligned(cnt, 4))
        return ISA_EALIGN;
    const Geo geo = geometry((long)L);
    hipLaunchKernelGGL(disc_means_kernel, dim3(n), dim3(1024), 0, as_stream(stream), slab, cslab, n_objects, cfg, geo.chunks, mu,
                       m, mnorm, cnt);
    return launch_status();
}

extern "C" int isa_disc_hinge(const isa_tensor* emb, const uint8_t* labels, int32_t k, const int32_t* n_objects,
                              const float* mu, const float* cfg, int32_t norm, float* hslab, double* partial, void* stream) {
    const int rc = emb_status(emb, CH);
    if (rc != ISA_OK) return rc;
    if (!labels || !n_objects || !mu || !cfg || !hslab || !partial || k < 1 || k > KI || (norm != 1 && norm != 2))
        return ISA_EINVAL;
    if (!aligned(n_objects, 4) || !aligned(mu, 16) || !aligned(cfg, 4) || !aligned(hslab, 16) || !aligned(partial, 8))
        return ISA_EALIGN;
    const Geo geo = geometry((long)emb->h * emb->w);
    const dim3 grid(geo.chunks, emb->n);
    hipStream_t st = as_stream(stream);
    by_dtype(emb->dtype, [&](auto t) { by_flag(norm == 2, [&](auto l2) {
        hipLaunchKernelGGL((disc_hinge_kernel<decltype(t), decltype(l2)::value ? 2 : 1>), grid, dim3(NT), 0, st, mkview(emb), labels, (int)k,
                           n_objects, mu, cfg, geo.per, hslab, partial);
    }); });
    return launch_status();
}

extern "C" int isa_disc_assemble(const float* hslab, const double* partial, const float* mu, const float* mnorm,
                                 const int32_t* cnt, const int32_t* n_objects, const float* cfg, int32_t norm, int32_t n,
                                 int64_t L, float* gconst, float* coef, double* img, float* scal, void* stream) {
    if (!hslab || !partial || !mu || !mnorm || !cnt || !n_objects || !cfg || !gconst || !coef || !img || !scal ||
        !batch_ok(n, L) || (norm != 1 && norm != 2))
        return ISA_EINVAL;
    if (!aligned(hslab, 16) || !aligned(partial, 8) || !aligned(mu, 16) || !aligned(mnorm, 4) || !aligned(cnt, 4) ||
        !aligned(n_objects, 4) || !aligned(cfg, 4) || !aligned(gconst, 16) || !aligned(coef, 4) || !aligned(img, 8) ||
        !aligned(scal, 4))
        return ISA_EALIGN;
    const Geo geo = geometry((long)L);
    hipStream_t st = as_stream(stream);
    by_flag(norm == 2, [&](auto l2) {
        hipLaunchKernelGGL((disc_image_kernel<decltype(l2)::value ? 2 : 1>), dim3(n), dim3(1024), 0, st, hslab, partial, mu, mnorm, cnt, n_objects,
                           cfg, (int)n, geo.chunks, gconst, coef, img);
    });
    hipLaunchKernelGGL(disc_total_kernel, dim3(1), dim3(64), 0, st, (const double*)img, cfg, (int)n, coef, scal);
    return launch_status();
}

extern "C" int isa_disc_grad(const isa_tensor* emb, const uint8_t* labels, int32_t k, const int32_t* n_objects,
                             const float* mu, const float* gconst, const float* coef, const float* cfg, int32_t norm,
                             const isa_tensor* demb, int32_t accumulate, void* stream) {
    const int rc = emb_status(emb, CH);
    if (rc != ISA_OK) return rc;
    if (!labels || !n_objects || !mu || !gconst || !coef || !cfg || !demb || !demb->data || k < 1 || k > KI ||
        (norm != 1 && norm != 2))
        return ISA_EINVAL;
    if (!same_shape(demb, emb) || demb->ld < demb->c || demb->ld % 8 || tensor_groups(demb) != 1) return ISA_EINVAL;
    if (!aligned(demb->data, 16) || !aligned(n_objects, 4) || !aligned(mu, 16) || !aligned(gconst, 16) || !aligned(coef, 4) ||
        !aligned(cfg, 4))
        return ISA_EALIGN;
    const long L = (long)emb->h * emb->w;
    const dim3 grid(grid_cap(cdiv(4 * L, NT), 256), emb->n);
    hipStream_t st = as_stream(stream);
    by_dtype(emb->dtype, [&](auto t) { by_flag(norm == 2, [&](auto l2) {
        hipLaunchKernelGGL((disc_grad_kernel<decltype(t), decltype(l2)::value ? 2 : 1>), grid, dim3(NT), 0, st, mkview(emb), labels, (int)k,
                           n_objects, mu, gconst, coef, cfg, mkview(demb), (int)accumulate);
    }); });
    return launch_status();
}
