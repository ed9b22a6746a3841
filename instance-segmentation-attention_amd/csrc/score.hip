// Scoring instance predictions on the device: Symmetric Best Dice, |difference in count| and foreground Dice
// (code/evaluate.py:18-56 of the reference) from the joint histogram of two uint8 label maps.
//   isa_labels_from_planes: ground-truth instance planes -> uint8 label map (the form ReSeg.segment writes);
//   isa_label_pair_hist   : hist[i][p][q] = #{pixels of image i with a == p and b == q}, int32, zeroed by the entry;
//   isa_instance_scores   : the eight scores of an image from its histogram, one workgroup per image, in double.
// The histogram pass has the shape of seg_claim_kernel (segment.hip): a row is cut into S <= ISA_ROW_CHUNKS chunks, one
// 256-thread workgroup each, the maps are read 4 or 16 pixels per load, a workgroup counts into an LDS histogram and adds
// its non-zero counters to hist with integer atomics - integer addition, so the result is the same whatever order the
// workgroups run in.
// Contention: leaf images are mostly background, so most pixels hit the ONE counter (0,0) and same-address LDS atomics
// serialise.  Per trip a wave elects the pair of its first lane's first pixel as the dominant pair; every pixel is
// compared with it, the matches are counted with ballot + popcount on the scalar unit and added once per wave and trip.
// The pixels that differ are run-length merged within the lane (equal consecutive pairs: one add) before the LDS atomic.
#include "common.hpp"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_MIN_CHUNK = 4096;
constexpr int SC_MAX_BINS = 16384;          // 64 KiB of int32 LDS counters
constexpr int SC_MAX_IDS = 256;             // labels are uint8

struct ScGeom { long L; int S; long chunk; };      // chunk: pixels per workgroup, a multiple of the trip

// W: 32-bit words of either map per lane and trip (1: 4 pixels, 4: 16 pixels in one 16-byte load)
bool sc_geom(int64_t L, int W, ScGeom* g) {
    const long trip = (long)SC_THREADS * 4 * W;
    if (L <= 0 || L % 4 || L > 0x7fffffffL - trip) return false;
    long S = (L + SC_MIN_CHUNK - 1) / SC_MIN_CHUNK;
    if (S > ISA_ROW_CHUNKS) S = ISA_ROW_CHUNKS;
    long chunk = (L + S - 1) / S;
    chunk = (chunk + trip - 1) / trip * trip;
    S = (L + chunk - 1) / chunk;
    *g = ScGeom{(long)L, (int)S, chunk};
    return true;
}

// ---- isa_labels_from_planes -----------------------------------------------------------------------------------------
// one thread per pixel; PIXEL_MAJOR: planes [n, hw, k] (the k values of a pixel are contiguous), else [n, k, hw]
template <typename T, bool PIXEL_MAJOR>
__global__ __launch_bounds__(SC_THREADS) void planes_kernel(const T* planes, int k, long hw, uint8_t* labels) {
    const long p = (long)blockIdx.x * SC_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= hw) return;
    const T* q = planes + (PIXEL_MAJOR ? ((long)b * hw + p) * k : (long)b * k * hw + p);
    const long step = PIXEL_MAJOR ? 1 : hw;
    int lab = 0;
    for (int j = 0; j < k; ++j) if (q[j * step] != (T)0) { lab = j + 1; break; }
    labels[(long)b * hw + p] = (uint8_t)lab;
}

// ---- isa_label_pair_hist --------------------------------------------------------------------------------------------
// NAIVE: one LDS atomic per pixel (the figure the aggregation is measured against; scripts/bench_score.py)
template <int W, bool NAIVE>
__global__ __launch_bounds__(SC_THREADS) void pair_hist_kernel(const uint8_t* a, const uint8_t* b, ScGeom g, int na, int nb,
                                                               int32_t* hist, int32_t* oob) {
    extern __shared__ int32_t bins[];
    const int s = blockIdx.x, img = blockIdx.y, lane = threadIdx.x & 63;
    const int nbins = na * nb;
    for (int i = threadIdx.x; i < nbins; i += SC_THREADS) bins[i] = 0;
    __syncthreads();
    const long p0 = (long)s * g.chunk, p1 = min(g.L, p0 + g.chunk);
    const uint8_t* ra = a + (long)img * g.L;
    const uint8_t* rb = b + (long)img * g.L;
    int n_oob = 0;                               // this lane's pixels outside [0, na) x [0, nb)
    int run_key = -1, run_len = 0;               // the lane's current run of equal pairs that are not the dominant one
    // the trip loop is wave-uniform (every lane runs every trip; a lane past the end holds no pixel), so that the
    // ballots below see the whole wave and lane 0 can speak for it
    for (long base = p0; base < p1; base += (long)SC_THREADS * 4 * W) {
        const long p = base + (long)threadIdx.x * 4 * W;
        uint32_t wa[W], wb[W];
        int words = 0;                           // valid words of this lane (L % 4 == 0: a word is whole or absent)
        if constexpr (W == 4) {
            if (p + 16 <= p1) {
                const uint4 va = *reinterpret_cast<const uint4*>(ra + p), vb = *reinterpret_cast<const uint4*>(rb + p);
                wa[0] = va.x; wa[1] = va.y; wa[2] = va.z; wa[3] = va.w;
                wb[0] = vb.x; wb[1] = vb.y; wb[2] = vb.z; wb[3] = vb.w;
                words = 4;
            } else {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    wa[w] = wb[w] = 0;
                    if (p + 4 * w < p1) {
                        wa[w] = *reinterpret_cast<const uint32_t*>(ra + p + 4 * w);
                        wb[w] = *reinterpret_cast<const uint32_t*>(rb + p + 4 * w);
                        words = w + 1;
                    }
                }
            }
        } else {
            wa[0] = wb[0] = 0;
            if (p < p1) {
                wa[0] = *reinterpret_cast<const uint32_t*>(ra + p);
                wb[0] = *reinterpret_cast<const uint32_t*>(rb + p);
                words = 1;
            }
        }
        // key of a pixel: its counter, -1 outside the histogram, -2 no pixel
        int key[4 * W];
#pragma unroll
        for (int w = 0; w < W; ++w)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int pa = (wa[w] >> (8 * j)) & 0xffu, pb = (wb[w] >> (8 * j)) & 0xffu;
                key[4 * w + j] = w >= words ? -2 : (pa < na && pb < nb) ? pa * nb + pb : -1;
            }
        if constexpr (NAIVE) {
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) {
                if (key[j] >= 0) atomicAdd(&bins[key[j]], 1);
                else if (key[j] == -1) ++n_oob;
            }
        } else {
            // the first lane of a wave past the end of the chunk holds no pixel: dom == -2 then matches nothing that counts
            const int dom = __builtin_amdgcn_readfirstlane(key[0]);
            int dom_count = 0;                                          // wave-uniform
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) dom_count += __popcll(__ballot(key[j] == dom));
#pragma unroll
            for (int j = 0; j < 4 * W; ++j) {
                if (key[j] == dom || key[j] == -2) continue;
                if (key[j] == -1) { ++n_oob; continue; }
                if (key[j] == run_key) { ++run_len; continue; }
                if (run_len) atomicAdd(&bins[run_key], run_len);
                run_key = key[j]; run_len = 1;
            }
            if (lane == 0) {
                if (dom >= 0) atomicAdd(&bins[dom], dom_count);
                else if (dom == -1) n_oob += dom_count;
            }
        }
    }
    if (run_len) atomicAdd(&bins[run_key], run_len);
    n_oob = wave_sum(n_oob);
    if (lane == 0 && n_oob) atomicAdd(oob + img, n_oob);
    __syncthreads();
    int32_t* out = hist + (long)img * nbins;
    for (int i = threadIdx.x; i < nbins; i += SC_THREADS) {
        const int v = bins[i];
        if (v) atomicAdd(out + i, v);
    }
}

// ---- isa_instance_scores --------------------------------------------------------------------------------------------
// best[p] = max over the objects q of the other map of 2 h / (size_p + size_q); a wave per object p, lanes over q.
// A_ROWS: p indexes rows of hist (a -> b), else columns (b -> a).  max over no object is 0.
template <bool A_ROWS>
__device__ __forceinline__ void best_dice(const int32_t* h, int np, int nq, int nb, const int* size_p, const int* size_q,
                                          double* best) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int p = 1 + wave; p < np; p += SC_THREADS / 64) {
        if (size_p[p] == 0) continue;                                    // wave-uniform
        double m = 0.0;
        for (int q = 1 + lane; q < nq; q += 64) {
            if (size_q[q] == 0) continue;
            const int v = A_ROWS ? h[p * nb + q] : h[q * nb + p];
            m = fmax(m, 2.0 * (double)v / ((double)size_p[p] + (double)size_q[q]));
        }
        m = wave_max(m);
        if (lane == 0) best[p] = m;
    }
}

__global__ __launch_bounds__(SC_THREADS) void scores_kernel(const int32_t* hist, int na, int nb, const int32_t* n_a,
                                                            const int32_t* n_b, double* out) {
    __shared__ int size_a[SC_MAX_IDS], size_b[SC_MAX_IDS];
    __shared__ double best_a[SC_MAX_IDS], best_b[SC_MAX_IDS];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int32_t* h = hist + (long)img * na * nb;
    size_a[tid] = 0; size_b[tid] = 0;                                    // SC_THREADS == SC_MAX_IDS
    __syncthreads();
    for (int i = tid; i < na * nb; i += SC_THREADS) {
        const int v = h[i];
        if (v) { atomicAdd(&size_a[i / nb], v); atomicAdd(&size_b[i % nb], v); }
    }
    __syncthreads();
    best_dice<true>(h, na, nb, nb, size_a, size_b, best_a);
    best_dice<false>(h, nb, na, nb, size_b, size_a, best_b);
    __syncthreads();
    if (tid != 0) return;
    // the sums run over the objects in label order: at most 255 values in [0, 1] each
    int objs_a = 0, objs_b = 0;
    long total = 0;
    double sum_a = 0.0, sum_b = 0.0;
    for (int p = 0; p < na; ++p) total += size_a[p];
    for (int p = 1; p < na; ++p) if (size_a[p]) { ++objs_a; sum_a += best_a[p]; }
    for (int q = 1; q < nb; ++q) if (size_b[q]) { ++objs_b; sum_b += best_b[q]; }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double bd_ab = objs_a ? sum_a / (double)objs_a : nan;
    const double bd_ba = objs_b ? sum_b / (double)objs_b : nan;
    const long fg_a = total - size_a[0], fg_b = total - size_b[0];
    const long both = total - size_a[0] - size_b[0] + h[0];              // inclusion-exclusion on the background
    const int cnt_a = n_a ? n_a[img] : objs_a, cnt_b = n_b ? n_b[img] : objs_b;
    double* o = out + (long)img * 8;
    o[0] = bd_ab;
    o[1] = bd_ba;
    o[2] = fmin(bd_ab, bd_ba);                                           // fmin: the number, if only one of them is NaN
    o[3] = (double)objs_a;
    o[4] = (double)objs_b;
    o[5] = fabs((double)cnt_a - (double)cnt_b);
    o[6] = (fg_a + fg_b) ? 2.0 * (double)both / ((double)fg_a + (double)fg_b) : nan;
    o[7] = 0.0;
}

bool ids_ok(int na, int nb) {
    return na >= 1 && na <= SC_MAX_IDS && nb >= 1 && nb <= SC_MAX_IDS && na * nb <= SC_MAX_BINS;
}

}  // namespace

extern "C" int isa_labels_from_planes(const void* planes, int32_t form, int32_t n, int32_t k, int64_t hw, uint8_t* labels,
                                      void* stream) {
    if (!planes || !labels || form < ISA_PLANES_U8_NHWK || form > ISA_PLANES_F32_NKHW || n <= 0 || n > 65535 || k < 1 ||
        k > 255 || hw <= 0 || hw > 0x7fffffffL - SC_THREADS)
        return ISA_EINVAL;
    if (!aligned(planes, form == ISA_PLANES_I64_NKHW ? 8 : form == ISA_PLANES_F32_NKHW ? 4 : 1)) return ISA_EALIGN;
    const dim3 grid(cdiv(hw, SC_THREADS), n), block(SC_THREADS);
    hipStream_t st = as_stream(stream);
    if (form == ISA_PLANES_U8_NHWK)
        hipLaunchKernelGGL((planes_kernel<uint8_t, true>), grid, block, 0, st, reinterpret_cast<const uint8_t*>(planes), k,
                           (long)hw, labels);
    else if (form == ISA_PLANES_I64_NKHW)
        hipLaunchKernelGGL((planes_kernel<int64_t, false>), grid, block, 0, st, reinterpret_cast<const int64_t*>(planes), k,
                           (long)hw, labels);
    else
        hipLaunchKernelGGL((planes_kernel<float, false>), grid, block, 0, st, reinterpret_cast<const float*>(planes), k,
                           (long)hw, labels);
    return launch_status();
}

extern "C" int isa_label_pair_hist(const uint8_t* a, const uint8_t* b, int32_t n, int64_t L, int32_t na, int32_t nb,
                                   int32_t* hist, int32_t* oob, int32_t mode, void* stream) {
    if (!a || !b || !hist || !oob || n <= 0 || n > 65535 || !ids_ok(na, nb) || L <= 0 || L % 4 ||
        (mode != ISA_HIST_AGGREGATE && mode != ISA_HIST_NAIVE))
        return ISA_EINVAL;
    if (!aligned(a, 4) || !aligned(b, 4) || !aligned(hist, 4) || !aligned(oob, 4)) return ISA_EALIGN;
    const bool wide = L % 16 == 0 && aligned(a, 16) && aligned(b, 16);
    ScGeom g;
    if (!sc_geom(L, wide ? 4 : 1, &g)) return ISA_EINVAL;
    hipStream_t st = as_stream(stream);
    const size_t lds = (size_t)na * nb * sizeof(int32_t);
    if (hipMemsetAsync(hist, 0, (size_t)n * lds, st) != hipSuccess || hipMemsetAsync(oob, 0, (size_t)n * 4, st) != hipSuccess)
        return ISA_ELAUNCH;
    const dim3 grid(g.S, n), block(SC_THREADS);
#define SC_LAUNCH(W, NV) hipLaunchKernelGGL((pair_hist_kernel<W, NV>), grid, block, lds, st, a, b, g, na, nb, hist, oob)
    if (mode == ISA_HIST_NAIVE) { if (wide) SC_LAUNCH(4, true); else SC_LAUNCH(1, true); }
    else { if (wide) SC_LAUNCH(4, false); else SC_LAUNCH(1, false); }
#undef SC_LAUNCH
    return launch_status();
}

extern "C" int isa_instance_scores(const int32_t* hist, int32_t n, int32_t na, int32_t nb, const int32_t* n_a,
                                   const int32_t* n_b, double* out, void* stream) {
    if (!hist || !out || n <= 0 || n > 65535 || !ids_ok(na, nb)) return ISA_EINVAL;
    if (!aligned(hist, 4) || !aligned(out, 8) || !aligned(n_a, 4) || !aligned(n_b, 4)) return ISA_EALIGN;
    hipLaunchKernelGGL(scores_kernel, dim3(n), dim3(SC_THREADS), 0, as_stream(stream), hist, na, nb, n_a, n_b, out);
    return launch_status();
}
