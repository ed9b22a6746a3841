// Scoring K-class semantic predictions on the device: confusion matrix, per-class IoU and Dice, mean IoU, pixel accuracy.
//   isa_sem_confusion: logits NHWC [n,h,w,K] -> class map (uint8, arg-max over the K channels) and / or the confusion
//                      matrix conf[i][label][prediction] (int64) against a uint8 label map, in ONE pass over the logits;
//   isa_sem_scores   : the 4 + 2K scores of an image (or of a summed matrix) from its confusion matrix, in double.
// The confusion pass has the row-chunk shape of pair_hist_kernel (score.hip) and seg_claim_kernel (segment.hip): a row is
// cut into S <= ISA_ROW_CHUNKS chunks of at least 4096 pixels, one 256-thread workgroup each.
// Logits: every lane issues one 16-byte load per round.  A pixel's K channels are EPV = 8 (bf16) or 4 (fp32) to the
// vector, so P = 1, 2, 4 or 8 neighbouring lanes share a pixel (the vectors of one pixel, then of the next: consecutive
// lanes read consecutive 16 bytes when ld == rup(K, 8)).  A lane takes the arg-max of its own vector, the P lanes of a
// pixel fold theirs with log2(P) DPP exchanges.  A trip is SM_ROUNDS rounds; the next trip's loads (logits and labels)
// are issued before this trip is worked on, so that a lane keeps that many loads in flight - with one workgroup of four
// waves per chunk nothing else hides the latency.  Channels c >= K (the ld padding) are never compared, and no load reaches past channel
// rup(K, 8) of a row.
// Labels and class ids: the first lane of every 4 pixels gathers the 4 predictions from its neighbours, writes them as
// one 32-bit word and reads the 4 labels as one.
// Counters: an int32 table [K][K] per WAVE in LDS (K^2 <= 1024: 16 KiB for the four), folded at the end; the workgroup
// adds its non-zero counters to conf with 64-bit integer atomics - integer addition, so the result is the same whatever
// order the workgroups run in.  Contention: semantic maps are mostly background, most pixels hit the ONE counter (0,0),
// and same-address LDS atomics serialise.  As in pair_hist_kernel: per round a wave elects the pair of its first pixel
// as the dominant one, counts the matches with ballot + popcount on the scalar unit and adds them once; the pixels that
// differ are run-length merged within the lane before the LDS atomic.
#include "common.hpp"

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_MIN_CHUNK = 4096;
constexpr int SM_ROUNDS = 8;                 // rounds (16-byte loads per lane) per trip
constexpr int SM_NONE = 1 << 20;             // channel index of "no candidate": loses every tie

struct SmGeom { long L; int S; long chunk; };      // chunk: pixels per workgroup, a multiple of the trip

// P: lanes per pixel.  A trip is SM_ROUNDS rounds of SM_THREADS / P pixels.
bool sm_geom(int64_t L, int P, SmGeom* g) {
    const long trip = (long)SM_ROUNDS * SM_THREADS / P;
    if (L <= 0 || L % 4 || L > 0x7fffffffL - trip) return false;
    long S = (L + SM_MIN_CHUNK - 1) / SM_MIN_CHUNK;
    if (S > ISA_ROW_CHUNKS) S = ISA_ROW_CHUNKS;
    long chunk = (L + S - 1) / S;
    chunk = (chunk + trip - 1) / trip * trip;
    S = (L + chunk - 1) / chunk;
    *g = SmGeom{(long)L, (int)S, chunk};
    return true;
}

template <typename T> struct vec16;
template <> struct vec16<bf16_t> {
    static constexpr int EPV = 8;
    bf16x8 v;
    __device__ __forceinline__ float get(int i) const { return (float)v[i]; }
};
template <> struct vec16<float> {
    static constexpr int EPV = 4;
    f32x4 v;
    __device__ __forceinline__ float get(int i) const { return v[i]; }
};

// is candidate (v, c) the arg-max rather than (bv, bc)?  NaN is the maximum, the lower channel wins a tie: a total order
// on candidates with distinct channels, so every lane of a pixel folds to the same one.
__device__ __forceinline__ bool sm_better(float v, int c, float bv, int bc) {
    const bool na = v != v, nb = bv != bv;
    return na ? (!nb || c < bc) : (!nb && (v > bv || (v == bv && c < bc)));
}

// DPP lane exchange inside a row of 16 lanes; a lane without a source keeps its own value
template <int CTRL> __device__ __forceinline__ int sm_dpp(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);
}
template <int CTRL> __device__ __forceinline__ void sm_fold(float& best, int& bi) {
    const float ov = __int_as_float(sm_dpp<CTRL>(__float_as_int(best)));
    const int oc = sm_dpp<CTRL>(bi);
    if (sm_better(ov, oc, best, bi)) { best = ov; bi = oc; }
}


template <typename T, int P>
__global__ __launch_bounds__(SM_THREADS) void sem_confusion_kernel(const T* logits, long ld, int K, const uint8_t* labels,
                                                                   SmGeom g, unsigned long long* conf, int32_t* oob,
                                                                   uint8_t* class_map) {
    constexpr int EPV = vec16<T>::EPV;
    constexpr int PPR = SM_THREADS / P;                 // pixels per round
    extern __shared__ int32_t sm_bins[];                // [SM_WAVES][K*K], only with labels
    const int s = blockIdx.x, img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nbins = K * K;
    int32_t* bins = sm_bins + wave * nbins;
    if (labels) {
        for (int i = tid; i < SM_WAVES * nbins; i += SM_THREADS) sm_bins[i] = 0;
        __syncthreads();
    }
    const long p0 = (long)s * g.chunk, p1 = min(g.L, p0 + g.chunk);
    const int sub = tid % P;                            // this lane's vector of its pixel
    const int c0 = sub * EPV;                           // first channel of that vector
    const bool has_vec = c0 < K;                        // else the vector is padding only (or past the row): not looked at
    const bool leader = tid % (4 * P) == 0;             // first lane of 4 consecutive pixels
    const T* row = logits + (long)img * g.L * ld + (has_vec ? c0 : 0);
    const uint8_t* lab_row = labels ? labels + (long)img * g.L : nullptr;
    uint8_t* map_row = class_map ? class_map + (long)img * g.L : nullptr;
    int n_oob = 0;
    int run_key = -1, run_len = 0;                      // the lane's current run of equal pairs that are not dominant
    // One trip's loads: SM_ROUNDS logit vectors and, with labels, as many label words.  No branch in front of a load: a
    // lane without a pixel or without a vector of its own re-reads one that exists (the chunk's last pixel, the pixel's
    // first vector) and drops it later; every lane of four pixels reads their label word (one address), the leader uses it.
    auto load_trip = [&](long base, vec16<T> (&raw)[SM_ROUNDS], uint32_t (&lw)[SM_ROUNDS]) {
#pragma unroll
        for (int u = 0; u < SM_ROUNDS; ++u) {
            const long q = min(base + u * PPR + tid / P, p1 - 1);
            raw[u].v = *reinterpret_cast<const decltype(raw[u].v)*>(row + q * ld);
            lw[u] = lab_row ? *reinterpret_cast<const uint32_t*>(lab_row + (q & ~3L)) : 0u;
        }
    };
    vec16<T> raw[SM_ROUNDS], nxt[SM_ROUNDS];
    uint32_t lw[SM_ROUNDS], lw_nxt[SM_ROUNDS];
    load_trip(p0, raw, lw);
    // the trip loop is wave-uniform (every lane runs every round; a lane past the end holds no pixel), so that the
    // lane exchanges and ballots below see the whole wave.  The next trip's loads are issued before this trip is worked on.
    for (long base = p0; base < p1; base += (long)SM_ROUNDS * PPR) {
        const bool more = base + (long)SM_ROUNDS * PPR < p1;        // workgroup-uniform
        if (more) load_trip(base + (long)SM_ROUNDS * PPR, nxt, lw_nxt);
#pragma unroll
        for (int u = 0; u < SM_ROUNDS; ++u) {
            const long q = base + u * PPR + tid / P;
            float best = has_vec ? raw[u].get(0) : -INFINITY;
            int bi = has_vec ? c0 : SM_NONE;
#pragma unroll
            for (int i = 1; i < EPV; ++i) {
                const float v = raw[u].get(i);
                // ascending channels: a later one wins only when strictly greater, or the first NaN
                if (c0 + i < K && (v > best || (v != v && best == best))) { best = v; bi = c0 + i; }
            }
            // the P lanes of a pixel sit in one row of 16 lanes: DPP exchanges, no LDS round trip
            if constexpr (P >= 2) sm_fold<0xB1>(best, bi);           // quad_perm [1,0,3,2]: lane ^ 1
            if constexpr (P >= 4) sm_fold<0x4E>(best, bi);           // quad_perm [2,3,0,1]: lane ^ 2
            if constexpr (P >= 8) sm_fold<0x141>(best, bi);          // row_half_mirror: the other quad of the 8 lanes
            // the four predictions of the leader's pixels q .. q+3 (q % 4 == 0; all four exist or none: L % 4 == 0)
            int b1, b2, b3;
            if constexpr (P <= 4) {
                b1 = sm_dpp<0x100 + P>(bi); b2 = sm_dpp<0x100 + 2 * P>(bi); b3 = sm_dpp<0x100 + 3 * P>(bi);   // row_shl
            } else {
                b1 = sm_dpp<0x100 + P>(bi); b2 = __shfl_down(bi, 2 * P, 64); b3 = __shfl_down(bi, 3 * P, 64);
            }
            const bool live = leader && q < p1;
            const int pr[4] = {bi, b1, b2, b3};
            if (live && map_row)
                *reinterpret_cast<uint32_t*>(map_row + q) = (uint32_t)bi | (uint32_t)b1 << 8 | (uint32_t)b2 << 16 | (uint32_t)b3 << 24;
            if (!lab_row) continue;                     // kernel-uniform
            const uint32_t lwu = lw[u];
            // key of a pixel: its counter, -1 label outside [0, K), -2 no pixel
            int key[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = (lwu >> (8 * j)) & 0xffu;
                key[j] = !live ? -2 : t < K ? t * K + pr[j] : -1;
            }
            // lane 0 of a wave is a leader; past the end of the chunk dom == -2 matches nothing that counts
            const int dom = __builtin_amdgcn_readfirstlane(key[0]);
            int dom_count = 0;                          // wave-uniform
#pragma unroll
            for (int j = 0; j < 4; ++j) dom_count += __popcll(__ballot(key[j] == dom));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
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
        if (more) {
#pragma unroll
            for (int u = 0; u < SM_ROUNDS; ++u) { raw[u] = nxt[u]; lw[u] = lw_nxt[u]; }
        }
    }
    if (!lab_row) return;
    if (run_len) atomicAdd(&bins[run_key], run_len);
    n_oob = wave_sum(n_oob);
    if (lane == 0 && n_oob) atomicAdd(oob + img, n_oob);
    __syncthreads();
    unsigned long long* out = conf + (long)img * nbins;
    for (int i = tid; i < nbins; i += SM_THREADS) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < SM_WAVES; ++w) v += sm_bins[w * nbins + i];
        if (v) atomicAdd(out + i, (unsigned long long)v);
    }
}

// one wave per image: lane c owns class c
__global__ __launch_bounds__(64) void sem_scores_kernel(const int64_t* conf, int K, double* out) {
    __shared__ double s_iou[ISA_SEM_MAX_CLASSES], s_dice[ISA_SEM_MAX_CLASSES];
    __shared__ long long s_tp[ISA_SEM_MAX_CLASSES], s_gt[ISA_SEM_MAX_CLASSES];
    __shared__ int s_present[ISA_SEM_MAX_CLASSES];
    const int img = blockIdx.x, c = threadIdx.x;
    const int64_t* m = conf + (long)img * K * K;
    double* o = out + (long)img * (4 + 2 * K);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (c < K) {
        long long gt = 0, pr = 0;
        for (int j = 0; j < K; ++j) { gt += m[c * K + j]; pr += m[j * K + c]; }
        const long long tp = m[c * K + c], uni = gt + pr - tp;
        const bool present = uni > 0;
        // exact integers below 2^53: each value is ONE correctly rounded division
        const double iou = present ? (double)tp / (double)uni : nan;
        const double dice = present ? (double)(2 * tp) / (double)(gt + pr) : nan;
        s_iou[c] = iou; s_dice[c] = dice; s_tp[c] = tp; s_gt[c] = gt; s_present[c] = present;
        o[4 + c] = iou;
        o[4 + K + c] = dice;
    }
    __syncthreads();
    if (c != 0) return;
    long long trace = 0, total = 0;
    int cnt = 0;
    double si = 0.0, sd = 0.0;                          // summed in class order: at most 32 values in [0, 1]
    for (int k = 0; k < K; ++k) {
        trace += s_tp[k]; total += s_gt[k];
        if (s_present[k]) { ++cnt; si += s_iou[k]; sd += s_dice[k]; }
    }
    o[0] = total ? (double)trace / (double)total : nan;
    o[1] = cnt ? si / (double)cnt : nan;
    o[2] = cnt ? sd / (double)cnt : nan;
    o[3] = (double)cnt;
}

template <typename T>
void sm_launch(int P, dim3 grid, size_t lds, hipStream_t st, const isa_tensor* x, const uint8_t* labels, SmGeom g,
               int64_t* conf, int32_t* oob, uint8_t* class_map) {
    const T* d = reinterpret_cast<const T*>(x->data);
    unsigned long long* cf = reinterpret_cast<unsigned long long*>(conf);
#define SM_LAUNCH(PP) hipLaunchKernelGGL((sem_confusion_kernel<T, PP>), grid, dim3(SM_THREADS), lds, st, d, (long)x->ld, \
                                         (int)x->c, labels, g, cf, oob, class_map)
    switch (P) {
        case 1: SM_LAUNCH(1); break;
        case 2: SM_LAUNCH(2); break;
        case 4: SM_LAUNCH(4); break;
        default: SM_LAUNCH(8); break;
    }
#undef SM_LAUNCH
}

}  // namespace

extern "C" int isa_sem_confusion(const isa_tensor* logits, const uint8_t* labels, int32_t K, int64_t* conf, int32_t* oob,
                                 uint8_t* class_map, void* stream) {
    if (!logits || !logits->data || (!labels && !class_map) || (labels && (!conf || !oob))) return ISA_EINVAL;
    if (K < 2 || K > ISA_SEM_MAX_CLASSES || logits->c != K || logits->n <= 0 || logits->n > 65535 || logits->h <= 0 ||
        logits->w <= 0 || logits->ld < logits->c || logits->ld % 8 || tensor_groups(logits) != 1)
        return ISA_EINVAL;
    const int64_t L = (int64_t)logits->h * logits->w;
    if (L % 4) return ISA_EINVAL;
    if (logits->dtype != ISA_F32 && logits->dtype != ISA_BF16) return ISA_EDTYPE;
    const int epv = logits->dtype == ISA_BF16 ? 8 : 4;
    const int nv = (K + epv - 1) / epv;                  // 16-byte vectors that hold a pixel's K channels
    const int P = nv <= 1 ? 1 : nv <= 2 ? 2 : nv <= 4 ? 4 : 8;
    SmGeom g;
    if (!sm_geom(L, P, &g)) return ISA_EINVAL;
    if (!aligned(logits->data, 16) || !aligned(labels, 4) || !aligned(class_map, 4) ||
        (labels && (!aligned(conf, 8) || !aligned(oob, 4))))
        return ISA_EALIGN;
    hipStream_t st = as_stream(stream);
    const int n = logits->n;
    size_t lds = 0;
    if (labels) {
        lds = (size_t)SM_WAVES * K * K * sizeof(int32_t);
        if (hipMemsetAsync(conf, 0, (size_t)n * K * K * sizeof(int64_t), st) != hipSuccess ||
            hipMemsetAsync(oob, 0, (size_t)n * sizeof(int32_t), st) != hipSuccess)
            return ISA_ELAUNCH;
    }
    const dim3 grid(g.S, n);
    by_dtype(logits->dtype, [&](auto t) { sm_launch<decltype(t)>(P, grid, lds, st, logits, labels, g, conf, oob, class_map); });
    return launch_status();
}

extern "C" int isa_sem_scores(const int64_t* conf, int32_t n, int32_t K, double* out, void* stream) {
    if (!conf || !out || n <= 0 || n > 65535 || K < 2 || K > ISA_SEM_MAX_CLASSES) return ISA_EINVAL;
    if (!aligned(conf, 8) || !aligned(out, 8)) return ISA_EALIGN;
    hipLaunchKernelGGL(sem_scores_kernel, dim3(n), dim3(64), 0, as_stream(stream), conf, (int)K, out);
    return launch_status();
}
