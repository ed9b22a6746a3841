// Clustering an instance embedding into instances (the inference side of the discriminative loss; reference:
// Prediction.cluster, code/lib/prediction.py:52-85, which runs sklearn KMeans on the host): greedy flat-kernel mean-shift and
// Lloyd's k-means, per image, on the device.  Semantics: include/isa_kernels.h and DESIGN.md section 16.
//
// emb x [B,H,W,C] NHWC (bf16 | fp32, C <= 32, ld a multiple of 8), fg uint8 [B, L = H*W] (non-zero = foreground), labels uint8
// [B, L] (0 background, 1..n instances).  d(p, c) = sum_j (x_p[j] - c[j])^2 is always the direct form: the difference, then one
// fp32 fmaf chain over the channels in order.  NaN embeddings are not supported (a NaN distance compares false everywhere).
//   init     per chunk: foreground count and smallest foreground index; clears the labels
//   ms pass  SHIFT: sum and count of the free pixels inside the ball; CLAIM: the ball takes label k + 1, the count and the
//            smallest index of what stays free; FINAL: the rest goes to its nearest centre (or to 0).  max_rounds rounds of
//            (shifts SHIFT + 1 CLAIM) are issued; a ball refused as noise has used up its round
//   far      one farthest-point pick per launch: (distance to the nearest chosen centre, index) arg-max, ties to the index
//   lloyd    a tile is staged in LDS once, assigned (VALU) and summed (one-hot[32 x P] . x[P x 32] on the f32-input MFMA)
// The host issues a fixed sequence of launches and reads nothing back.  What a pass hands to the next one - chunk sums,
// counts, minima - lies in per-chunk slabs, and every workgroup of the next pass folds them itself, in chunk order, in its
// prologue; workgroup 0 of an image also stores the folded state for the pass after that.  Slabs, state and centres are
// double-buffered by the parity of the launch, so nobody reads what the same launch writes.  No float atomics, no spin waits,
// no grid barriers: labels, counts and centres are bit-reproducible.  A finished image's workgroups return in the prologue.
#include "common.hpp"

#include <climits>
#include <cmath>

namespace {

constexpr int NT = 256, NW = 4, TP = 64, KI = ISA_DISC_MAX_K, CH = 32, XS = CH + 1, SLAB = KI * CH;
constexpr int CS = ISA_CLUSTER_CSLAB_STRIDE, STATE = ISA_CLUSTER_STATE_INTS;
constexpr int C_CNT = 32, C_MIN = 33, C_VAL = 34, C_IDX = 35;       // cslab columns past the 32 cluster counts
constexpr int NOISE = 255;
enum { MS_SHIFT = 0, MS_CLAIM = 1, MS_FINAL = 2 };
enum { PEND_NONE = 0, PEND_CLAIM = 1, PEND_INIT = 2 };


struct Geo { int chunks; long per; };
static inline Geo geometry(long L) {
    const int ch = (int)ISA_DISC_CHUNKS(L);
    return Geo{ch, ((L + ch - 1) / ch + TP - 1) / TP * TP};
}

// state int32 [2][B][16]: mean-shift {k, done, seed, pend}, k-means {K, foreground pixels} (parity 0 only)
// cen float [2][B][32][32]: mean-shift row 0 = the moving centre; k-means the centres of launch parity
// slab float [2][B][chunks][32][32], cslab int32 [2][B][chunks][36], acnt int32 [B][chunks][2] = {fg count, smallest fg index}
struct Scratch { int32_t* state; float* cen; float* slab; int32_t* cslab; int32_t* acnt; };
static inline Scratch carve(void* p, long n, long chunks) {
    Scratch s;
    char* c = reinterpret_cast<char*>(p);
    s.state = reinterpret_cast<int32_t*>(c); c += 2 * n * STATE * 4;
    s.cen = reinterpret_cast<float*>(c);     c += 2 * n * SLAB * 4;
    s.slab = reinterpret_cast<float*>(c);    c += 2 * n * chunks * SLAB * 4;
    s.cslab = reinterpret_cast<int32_t*>(c); c += 2 * n * chunks * CS * 4;
    s.acnt = reinterpret_cast<int32_t*>(c);
    return s;
}

__device__ __forceinline__ int clamp_nb(int v) { return v < 0 ? 0 : (v > KI ? KI : v); }

// 8 channels [8g, 8g+8) of a pixel row; channels >= c and groups past the last read as 0
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

// the wave's 64 pixels [base, base + 64) of image row0 / L -> xs[64][33]; pixels at or past p1 are zeros
template <typename T>
__device__ __forceinline__ void stage(const View& x, long row0, long base, long p1, float (*xs)[XS], int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int item = q * 64 + lane, px = item >> 2, g = item & 3;
        float v[8];
        if (base + px < p1) load_group<T>(x, row0 + base + px, g, v);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) xs[px][8 * g + i] = v[i];
    }
}
__device__ __forceinline__ void load_row(const float (*xs)[XS], int lane, float (&xr)[CH]) {
#pragma unroll
    for (int j = 0; j < CH; ++j) xr[j] = xs[lane][j];
}
// the direct form: channels past C are 0 on both sides and add an exact 0
__device__ __forceinline__ float dist32(const float (&xr)[CH], const float* c) {
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        const float t = xr[j] - c[j];
        d = fmaf(t, t, d);
    }
    return d;
}
// channel j (< 32) of pixel p of image b as float, 0 past C
template <typename T>
__device__ __forceinline__ float pixel_chan(const View& x, long row, int j) {
    return j < x.c ? (float)reinterpret_cast<const T*>(x.data)[row * x.ld + j] : 0.f;
}

// grid (chunks, B)
__global__ __launch_bounds__(NT) void cluster_init_kernel(const uint8_t* __restrict__ fg, uint8_t* __restrict__ labels, long L,
                                                          long per, Scratch s) {
    __shared__ int red[NW][2];
    const int b = blockIdx.y, chunk = blockIdx.x, nch = gridDim.x, B = gridDim.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long p0 = (long)chunk * per, p1 = p0 + per < L ? p0 + per : L;
    int cnt = 0, mn = INT_MAX;
    for (long p = p0 + threadIdx.x; p < p1; p += NT) {
        labels[(long)b * L + p] = 0;
        if (fg[(long)b * L + p]) { ++cnt; if ((int)p < mn) mn = (int)p; }
    }
    cnt = wave_sum(cnt);
    mn = wave_min(mn);
    if (lane == 0) { red[wave][0] = cnt; red[wave][1] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0, m = INT_MAX;
        for (int w = 0; w < NW; ++w) { c += red[w][0]; m = red[w][1] < m ? red[w][1] : m; }
        int32_t* a = s.acnt + ((long)b * nch + chunk) * 2;
        a[0] = c;
        a[1] = m;
    }
    if (chunk == 0 && threadIdx.x < STATE) {
        const int t = threadIdx.x;
        s.state[(long)b * STATE + t] = t == 2 ? -1 : (t == 3 ? PEND_INIT : 0);        // parity 0
        s.state[((long)B + b) * STATE + t] = 0;
    }
}

// One pass of the greedy mean-shift.  grid (chunks, B); q = index of the launch (the init launch is 0).  first: the pass
// opens an object (it follows the init or a CLAIM pass), else it follows a SHIFT pass of the same object.
template <typename T, int KIND>
__global__ __launch_bounds__(NT) void cluster_ms_kernel(View x, const uint8_t* __restrict__ fg, uint8_t* __restrict__ labels,
                                                        int first, int q, float bw2, int max_objects, int min_pixels,
                                                        int assign_rest, long per, Scratch s, float* __restrict__ centres,
                                                        int32_t* __restrict__ sizes, int32_t* __restrict__ n_objects,
                                                        int32_t* __restrict__ moved) {
    __shared__ float xs[NW][TP][XS];
    __shared__ float cs[KIND == MS_FINAL ? KI : 1][CH];
    __shared__ float redf[NW][CH];
    __shared__ int redi[NW][2];
    const int b = blockIdx.y, chunk = blockIdx.x, nch = gridDim.x, B = gridDim.y;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long L = (long)x.h * x.w, p0 = (long)chunk * per, p1 = p0 + per < L ? p0 + per : L;
    const int pin = (q & 1) ^ 1, pout = q & 1;
    const int32_t* stp = s.state + ((long)pin * B + b) * STATE;
    const float* cprev = s.cen + ((long)pin * B + b) * SLAB;
    const int32_t* csp = s.cslab + ((long)pin * B + b) * nch * CS;
    const float* slp = s.slab + ((long)pin * B + b) * nch * SLAB;
    int k = stp[0], done = stp[1], seed = stp[2];
    const int pend = stp[3];
    int fixv = 0, accepted = 0;                    // fixv: the label of a refused ball, to be rewritten as noise
    // ---- prologue: fold what the previous pass left (the same values in every thread and every workgroup)
    if (first) {
        if (pend == PEND_CLAIM) {
            int cnt = 0, ms = INT_MAX;
            for (int ch = 0; ch < nch; ++ch) {
                cnt += csp[ch * CS + C_CNT];
                const int m = csp[ch * CS + C_MIN];
                ms = m < ms ? m : ms;
            }
            if (cnt >= min_pixels) {
                if (chunk == 0 && t < CH) centres[((long)b * KI + k) * CH + t] = cprev[t];
                if (chunk == 0 && t == 0) sizes[b * KI + k] = cnt;
                ++k;
                accepted = 1;
            } else {
                fixv = k + 1;
            }
            seed = ms == INT_MAX ? -1 : ms;
        } else if (pend == PEND_INIT) {
            int ms = INT_MAX;
            for (int ch = 0; ch < nch; ++ch) {
                const int m = s.acnt[((long)b * nch + ch) * 2 + 1];
                ms = m < ms ? m : ms;
            }
            seed = ms == INT_MAX ? -1 : ms;
        }
        if (seed < 0 || k >= max_objects) done = 1;
        if (KIND != MS_FINAL && !done && t < CH) cs[0][t] = pixel_chan<T>(x, (long)b * L + seed, t);
    } else if (!done && t < CH) {
        int cnt = 0;
        float sum = 0.f;
        for (int ch = 0; ch < nch; ++ch) {
            cnt += csp[ch * CS + C_CNT];
            sum += slp[(long)ch * SLAB + t];
        }
        cs[0][t] = cnt > 0 ? sum / (float)cnt : cprev[t];
    }
    if (KIND == MS_FINAL) {
        for (int e = t; e < k * CH; e += NT)
            (&cs[0][0])[e] = (accepted && e >= (k - 1) * CH) ? cprev[e - (k - 1) * CH] : centres[(long)b * SLAB + e];
    }
    __syncthreads();
    if (chunk == 0) {
        if (t < STATE) {
            const int v = t == 0 ? k : (t == 1 ? done : (t == 2 ? seed : (t == 3 && !done && KIND == MS_CLAIM ? PEND_CLAIM : 0)));
            s.state[((long)pout * B + b) * STATE + t] = v;
        }
        if (KIND != MS_FINAL && !done && t < CH) s.cen[((long)pout * B + b) * SLAB + t] = cs[0][t];
    }
    if (KIND == MS_FINAL) {
        if (chunk == 0) {
            if (t == 0) { n_objects[b] = k; moved[b] = 0; }
            for (int e = k * CH + t; e < SLAB; e += NT) centres[(long)b * SLAB + e] = 0.f;
            if (t >= k && t < KI) sizes[b * KI + t] = 0;
        }
        const bool rest = assign_rest && k > 0;
        const int rounds = (int)((per + NW * TP - 1) / (NW * TP));
        for (int r = 0; r < rounds; ++r) {
            const long base = p0 + ((long)r * NW + wave) * TP;
            if (rest) {
                __syncthreads();
                stage<T>(x, (long)b * L, base, p1, xs[wave], lane);
                __syncthreads();
            }
            const long p = base + lane;
            if (p < p1) {
                const long gi = (long)b * L + p;
                const int lab = labels[gi];
                int out = 0;
                if (fg[gi]) {
                    if (lab >= 1 && lab <= k) out = lab;
                    else if (rest) {
                        float xr[CH];
                        load_row(xs[wave], lane, xr);
                        float best = dist32(xr, cs[0]);
                        out = 1;
                        for (int c = 1; c < k; ++c) {
                            const float d = dist32(xr, cs[c]);
                            if (d < best) { best = d; out = c + 1; }
                        }
                    }
                }
                if (out != lab) labels[gi] = (uint8_t)out;
            }
        }
        return;
    }
    if (done) return;
    // ---- body
    float acc[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) acc[j] = 0.f;
    int cnt = 0, mn = INT_MAX;
    const int rounds = (int)((per + NW * TP - 1) / (NW * TP));
    for (int r = 0; r < rounds; ++r) {
        const long base = p0 + ((long)r * NW + wave) * TP;
        __syncthreads();
        stage<T>(x, (long)b * L, base, p1, xs[wave], lane);
        __syncthreads();
        const long p = base + lane;
        if (p < p1) {
            const long gi = (long)b * L + p;
            int lab = labels[gi];
            if (fixv && lab == fixv) { lab = NOISE; labels[gi] = NOISE; }
            if (lab == 0 && fg[gi]) {
                float xr[CH];
                load_row(xs[wave], lane, xr);
                const float d = dist32(xr, cs[0]);
                if (KIND == MS_SHIFT) {
                    if (d <= bw2) {
                        ++cnt;
#pragma unroll
                        for (int j = 0; j < CH; ++j) acc[j] += xr[j];
                    }
                } else {
                    if (d <= bw2 || (int)p == seed) { labels[gi] = (uint8_t)(k + 1); ++cnt; }
                    else if ((int)p < mn) mn = (int)p;
                }
            }
        }
    }
    cnt = wave_sum(cnt);
    mn = wave_min(mn);
    if (lane == 0) { redi[wave][0] = cnt; redi[wave][1] = mn; }
    if (KIND == MS_SHIFT) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const float v = wave_sum(acc[j]);
            if (lane == 0) redf[wave][j] = v;
        }
    }
    __syncthreads();
    const long o = ((long)pout * B + b) * nch + chunk;
    if (t == 0) {
        int c = 0, m = INT_MAX;
        for (int w = 0; w < NW; ++w) { c += redi[w][0]; m = redi[w][1] < m ? redi[w][1] : m; }
        s.cslab[o * CS + C_CNT] = c;
        s.cslab[o * CS + C_MIN] = m;
    }
    if (KIND == MS_SHIFT && t < CH) s.slab[o * SLAB + t] = ((redf[0][t] + redf[1][t]) + redf[2][t]) + redf[3][t];
}

// K_b of the k-means passes from the init launch's counts
__device__ __forceinline__ int fold_K(const Scratch& s, int b, int nch, int nobj, int kmax, int& nfg) {
    int c = 0;
    for (int ch = 0; ch < nch; ++ch) c += s.acnt[((long)b * nch + ch) * 2];
    nfg = c;
    int K = clamp_nb(nobj);
    K = K < c ? K : c;
    return K < kmax ? K : kmax;
}

// Farthest-point launch j = 1 .. kmax: adopts centre j - 1 (the pick of launch j - 1; launch 1: the smallest foreground
// index), then picks centre j.  grid (chunks, B).  Centres go to cen parity 0, row by row.
template <typename T>
__global__ __launch_bounds__(NT) void cluster_far_kernel(View x, const uint8_t* __restrict__ fg,
                                                         const int32_t* __restrict__ nobj, int j, int kmax, long per,
                                                         Scratch s) {
    __shared__ float xs[NW][TP][XS];
    __shared__ float cs[KI][CH];
    __shared__ float redv[NW];
    __shared__ int redx[NW];
    const int b = blockIdx.y, chunk = blockIdx.x, nch = gridDim.x, B = gridDim.y;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long L = (long)x.h * x.w, p0 = (long)chunk * per, p1 = p0 + per < L ? p0 + per : L;
    int K;
    if (j == 1) {
        int nfg;
        K = fold_K(s, b, nch, nobj[b], kmax, nfg);
        if (chunk == 0 && t == 0) { s.state[(long)b * STATE] = K; s.state[(long)b * STATE + 1] = nfg; }
    } else {
        K = s.state[(long)b * STATE];
    }
    if (j - 1 >= K) return;
    int idx = INT_MAX;
    if (j == 1) {
        for (int ch = 0; ch < nch; ++ch) {
            const int m = s.acnt[((long)b * nch + ch) * 2 + 1];
            idx = m < idx ? m : idx;
        }
    } else {
        const int32_t* csp = s.cslab + ((long)((j - 1) & 1) * B + b) * nch * CS;
        float bv = -1.f;
        for (int ch = 0; ch < nch; ++ch) {
            const float v = __int_as_float(csp[ch * CS + C_VAL]);
            const int i = csp[ch * CS + C_IDX];
            if (v > bv || (v == bv && i < idx)) { bv = v; idx = i; }
        }
    }
    if (idx < 0 || idx >= L) idx = 0;             // (cannot happen: K_b >= 1 means a foreground pixel exists)
    float* cen0 = s.cen + (long)b * SLAB;
    for (int e = t; e < (j - 1) * CH; e += NT) (&cs[0][0])[e] = cen0[e];
    if (t < CH) {
        const float v = pixel_chan<T>(x, (long)b * L + idx, t);
        cs[j - 1][t] = v;
        if (chunk == 0) cen0[(j - 1) * CH + t] = v;
    }
    if (j >= K) return;
    float bv = -1.f;
    int bi = INT_MAX;
    const int rounds = (int)((per + NW * TP - 1) / (NW * TP));
    for (int r = 0; r < rounds; ++r) {
        const long base = p0 + ((long)r * NW + wave) * TP;
        __syncthreads();
        stage<T>(x, (long)b * L, base, p1, xs[wave], lane);
        __syncthreads();
        const long p = base + lane;
        if (p < p1 && fg[(long)b * L + p]) {
            float xr[CH];
            load_row(xs[wave], lane, xr);
            float dm = dist32(xr, cs[0]);
            for (int c = 1; c < j; ++c) dm = fminf(dm, dist32(xr, cs[c]));
            if (dm > bv) { bv = dm; bi = (int)p; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { redv[wave] = bv; redx[wave] = bi; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < NW; ++w)
            if (redv[w] > bv || (redv[w] == bv && redx[w] < bi)) { bv = redv[w]; bi = redx[w]; }
        const long o = ((long)(j & 1) * B + b) * nch + chunk;
        s.cslab[o * CS + C_VAL] = __float_as_int(bv);
        s.cslab[o * CS + C_IDX] = bi;
    }
}

// acc[i][c] += sum over the tile's 64 pixels of [lab == i + 1] * xs[pixel][c] (the lane layout of disc.hip's onehot_mma)
__device__ __forceinline__ void onehot_mma(const float (*xs)[XS], const int* labs, int lane, f32x16& acc) {
    const int half = lane >> 5, col = lane & 31;
#pragma unroll 8
    for (int s = 0; s < TP / 2; ++s) {
        const int px = 2 * s + half;
        const float a = labs[px] == col + 1 ? 1.f : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xs[px][col], acc, 0, 0, 0);
    }
}

// Lloyd launch i = 0 .. iters: the centres of iteration i (launch 0: cen_in; later: the means of launch i - 1's clusters, an
// empty cluster keeps its centre), the assignment, and the sums for launch i + 1.  grid (chunks, B).
template <typename T>
__global__ __launch_bounds__(NT) void cluster_lloyd_kernel(View x, const uint8_t* __restrict__ fg, uint8_t* __restrict__ labels,
                                                           const int32_t* __restrict__ nobj, const float* __restrict__ cen_in,
                                                           int given, int i, int kmax, long per, Scratch s) {
    __shared__ __attribute__((aligned(16))) float xs[NW][TP][XS];
    __shared__ float cs[KI][CH];
    __shared__ int labs[NW][TP];
    __shared__ int cnt[KI];
    __shared__ int redm[NW];
    const int b = blockIdx.y, chunk = blockIdx.x, nch = gridDim.x, B = gridDim.y;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long L = (long)x.h * x.w, p0 = (long)chunk * per, p1 = p0 + per < L ? p0 + per : L;
    int K;
    if (i == 0 && given) {
        int nfg;
        K = fold_K(s, b, nch, nobj[b], kmax, nfg);
        if (chunk == 0 && t == 0) { s.state[(long)b * STATE] = K; s.state[(long)b * STATE + 1] = nfg; }
    } else {
        K = s.state[(long)b * STATE];
    }
    if (K == 0) return;
    float* cout = s.cen + ((long)(i & 1) * B + b) * SLAB;
    if (i == 0) {
        for (int e = t; e < K * CH; e += NT) {
            const float v = (e & 31) < x.c ? cen_in[(long)b * SLAB + e] : 0.f;
            (&cs[0][0])[e] = v;
            if (chunk == 0 && given) cout[e] = v;
        }
    } else {
        const int pin = (i & 1) ^ 1;
        const float* cprev = s.cen + ((long)pin * B + b) * SLAB;
        const int32_t* csp = s.cslab + ((long)pin * B + b) * nch * CS;
        const float* slp = s.slab + ((long)pin * B + b) * nch * SLAB;
        for (int e = t; e < K * CH; e += NT) {
            int N = 0;
            float sum = 0.f;
            for (int ch = 0; ch < nch; ++ch) {
                N += csp[ch * CS + (e >> 5)];
                sum += slp[(long)ch * SLAB + e];
            }
            const float v = N > 0 ? sum / (float)N : cprev[e];
            (&cs[0][0])[e] = v;
            if (chunk == 0) cout[e] = v;
        }
    }
    if (t < KI) cnt[t] = 0;
    f32x16 acc = {};
    int mv = 0;
    const int rounds = (int)((per + NW * TP - 1) / (NW * TP));
    for (int r = 0; r < rounds; ++r) {
        const long base = p0 + ((long)r * NW + wave) * TP;
        __syncthreads();
        stage<T>(x, (long)b * L, base, p1, xs[wave], lane);
        __syncthreads();
        const long p = base + lane;
        int lab = 0;
        if (p < p1) {
            const long gi = (long)b * L + p;
            if (fg[gi]) {
                float xr[CH];
                load_row(xs[wave], lane, xr);
                float best = dist32(xr, cs[0]);
                lab = 1;
                for (int c = 1; c < K; ++c) {
                    const float d = dist32(xr, cs[c]);
                    if (d < best) { best = d; lab = c + 1; }
                }
                atomicAdd(&cnt[lab - 1], 1);
            }
            const int old = labels[gi];
            if (old != lab) { labels[gi] = (uint8_t)lab; ++mv; }
        }
        labs[wave][lane] = lab;
        __syncthreads();
        onehot_mma(xs[wave], labs[wave], lane, acc);
    }
    mv = wave_sum(mv);
    if (lane == 0) redm[wave] = mv;
    __syncthreads();
    const long o = ((long)(i & 1) * B + b) * nch + chunk;
    if (t < KI) s.cslab[o * CS + t] = cnt[t];
    if (t == 0) s.cslab[o * CS + C_CNT] = i > 0 ? redm[0] + redm[1] + redm[2] + redm[3] : 0;
    // the four waves' accumulators -> the chunk's slab, in wave order (xs is free: every wave is past its last tile)
    float* red = &xs[0][0][0];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        red[wave * SLAB + row * CH + (lane & 31)] = acc[r];
    }
    __syncthreads();
    float* out = s.slab + o * SLAB;
    for (int e = t; e < SLAB; e += NT) out[e] = ((red[e] + red[SLAB + e]) + red[2 * SLAB + e]) + red[3 * SLAB + e];
}

// grid B, 1024 threads: thread (row, channel)
__global__ __launch_bounds__(1024) void cluster_kmeans_out_kernel(Scratch s, int nch, int iters, float* __restrict__ centres,
                                                                  int32_t* __restrict__ sizes, int32_t* __restrict__ n_objects,
                                                                  int32_t* __restrict__ moved) {
    const int b = blockIdx.x, B = gridDim.x, t = threadIdx.x, row = t >> 5, j = t & 31;
    const int K = s.state[(long)b * STATE], par = iters & 1;
    const int32_t* csp = s.cslab + ((long)par * B + b) * nch * CS;
    centres[(long)b * SLAB + t] = row < K ? s.cen[((long)par * B + b) * SLAB + t] : 0.f;
    if (j == 0) {
        int N = 0;
        if (row < K)
            for (int ch = 0; ch < nch; ++ch) N += csp[ch * CS + row];
        sizes[b * KI + row] = N;
    }
    if (t == 0) {
        int m = 0;
        if (K > 0)
            for (int ch = 0; ch < nch; ++ch) m += csp[ch * CS + C_CNT];
        moved[b] = m;
        n_objects[b] = K;
    }
}

static_assert(NW * SLAB <= NW * TP * XS, "the accumulator fold reuses the tile buffer");

// the arguments both entries share
int common_status(const isa_tensor* emb, const uint8_t* fg, const uint8_t* labels, const int32_t* n_objects,
                  const float* centres, const int32_t* sizes, const int32_t* moved, const void* scratch) {
    const int rc = emb_status(emb, CH);
    if (rc != ISA_OK) return rc;
    if (!fg || !labels || !n_objects || !centres || !sizes || !moved || !scratch) return ISA_EINVAL;
    if (!aligned(n_objects, 4) || !aligned(centres, 16) || !aligned(sizes, 4) || !aligned(moved, 4) || !aligned(scratch, 16))
        return ISA_EALIGN;
    return ISA_OK;
}

}  // namespace

extern "C" int isa_cluster_meanshift(const isa_tensor* emb, const uint8_t* fg, float bandwidth, int32_t shifts,
                                     int32_t max_objects, int32_t max_rounds, int32_t min_pixels, int32_t assign_rest,
                                     uint8_t* labels,
                                     int32_t* n_objects, float* centres, int32_t* sizes, int32_t* moved, void* scratch,
                                     void* stream) {
    const int rc = common_status(emb, fg, labels, n_objects, centres, sizes, moved, scratch);
    if (rc != ISA_OK) return rc;
    if (!(bandwidth > 0.f) || !std::isfinite(bandwidth) || shifts < 0 || shifts > ISA_CLUSTER_MAX_SHIFTS || max_objects < 1 ||
        max_objects > KI || max_rounds < max_objects || max_rounds > ISA_CLUSTER_MAX_ROUNDS || min_pixels < 1)
        return ISA_EINVAL;
    const long L = (long)emb->h * emb->w;
    const Geo geo = geometry(L);
    const Scratch s = carve(scratch, emb->n, geo.chunks);
    const dim3 grid(geo.chunks, emb->n);
    hipStream_t st = as_stream(stream);
    const View v = mkview(emb);
    const float bw2 = bandwidth * bandwidth;
    hipLaunchKernelGGL(cluster_init_kernel, grid, dim3(NT), 0, st, fg, labels, L, geo.per, s);
    int q = 1;
    auto ms = [&](auto kind, bool first) {
        by_dtype(emb->dtype, [&](auto t) {
            hipLaunchKernelGGL((cluster_ms_kernel<decltype(t), decltype(kind)::value>), grid, dim3(NT), 0, st, v, fg, labels, (int)first, q,
                               bw2, (int)max_objects, (int)min_pixels, (int)assign_rest, geo.per, s, centres, sizes, n_objects, moved);
        });
        ++q;
    };
    // a round opens with a seed and ends with a ball that becomes an object or noise: the budget counts both kinds
    for (int round = 0; round < max_rounds; ++round) {
        for (int t = 0; t < shifts; ++t) ms(std::integral_constant<int, MS_SHIFT>{}, t == 0);
        ms(std::integral_constant<int, MS_CLAIM>{}, shifts == 0);
    }
    ms(std::integral_constant<int, MS_FINAL>{}, true);
    return launch_status();
}

extern "C" int isa_cluster_kmeans(const isa_tensor* emb, const uint8_t* fg, const int32_t* n_objects_in, const float* init,
                                  int32_t kmax, int32_t iters, uint8_t* labels, int32_t* n_objects, float* centres,
                                  int32_t* sizes, int32_t* moved, void* scratch, void* stream) {
    const int rc = common_status(emb, fg, labels, n_objects, centres, sizes, moved, scratch);
    if (rc != ISA_OK) return rc;
    if (!n_objects_in || kmax < 1 || kmax > KI || iters < 0 || iters > ISA_CLUSTER_MAX_ITERS) return ISA_EINVAL;
    if (!aligned(n_objects_in, 4) || !aligned(init, 16)) return ISA_EALIGN;
    const long L = (long)emb->h * emb->w;
    const Geo geo = geometry(L);
    const Scratch s = carve(scratch, emb->n, geo.chunks);
    const dim3 grid(geo.chunks, emb->n);
    hipStream_t st = as_stream(stream);
    const View v = mkview(emb);
    hipLaunchKernelGGL(cluster_init_kernel, grid, dim3(NT), 0, st, fg, labels, L, geo.per, s);
    const float* cen_in = init ? init : s.cen;
    by_dtype(emb->dtype, [&](auto t) {
        if (!init)
            for (int j = 1; j <= kmax; ++j)
                hipLaunchKernelGGL(cluster_far_kernel<decltype(t)>, grid, dim3(NT), 0, st, v, fg, n_objects_in, j, (int)kmax, geo.per, s);
        for (int i = 0; i <= iters; ++i)
            hipLaunchKernelGGL(cluster_lloyd_kernel<decltype(t)>, grid, dim3(NT), 0, st, v, fg, labels, n_objects_in, cen_in,
                               init ? 1 : 0, i, (int)kmax, geo.per, s);
    });
    hipLaunchKernelGGL(cluster_kmeans_out_kernel, dim3(emb->n), dim3(1024), 0, st, s, geo.chunks, (int)iters, centres, sizes,
                       n_objects, moved);
    return launch_status();
}
