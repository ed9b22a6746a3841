// Lovasz-Softmax semantic criterion (reference: lovasz_softmax / lovasz_softmax_flat / lovasz_grad,
// code/lib/losses/lovasz_losses.py:17-30,156-196) on the segmented sort of seg_sort.hip.
//
// logits l [B,H,W,K] NHWC (bf16 | fp32, ld = rup(K, 8)), labels y uint8 [B,H,W], p = softmax_c(l) in fp32.  For class c
// and pixel i: fg = [y_i == c], e = |fg - p_c(i)| clamped to [0, 1].  A segment is (class, whole batch), or (class, image)
// when per_image; both are ranges of the same array [K][B][H*W].  Per segment, with the errors in descending order
// (ties by ascending pixel index), G foreground pixels, and cf / cb the foreground / background pixels strictly
// earlier in that order, I = G - cf, U = G + cb:
//     g_r = 1/U (foreground) | I / (U (U+1)) (background) | G == 0: [r == 0]        loss_seg = sum_r e_r g_r
// which is jaccard[r] - jaccard[r-1] of lovasz_grad without its cancellation.
//   keys      key = 0x3F800000 - bits(e) (ascending key = descending error, 30 bits), value = pixel index in the segment
//             with fg in bit 31; G per segment with integer atomics
//   (isa_segsort_kv_u32 over bits [0, 30))
//   coef      three launches: foreground count of every tile of the sorted order, exclusive scan per segment, then per
//             element g_r from the integer counts (double), the tile's partial loss (double, fixed fold order) and
//             sign * g_r scattered back to pixel order (sign = d e / d p: -1 foreground, +1 background)
//   assemble  one workgroup: counted classes = optimize_bg ? 0..K-1 : 1..K-1, of which only_present keeps those with
//             G > 0 in the segment; loss = mean over the kept classes (0 when none), then over the images when
//             per_image; scale[c][segment] = 1 / (kept * images) for a kept class, else 0
//   grad      d_c = scale * sign * g;  d l_k = p_k (d_k - sum_j p_j d_j), evaluated around the likeliest class
// optimize_bg = cfg[2] and only_present = cfg[3] are read from the criterion's device buffer at run time; per_image sets
// the segment geometry and is a host argument.  No float atomics anywhere: loss and gradient are bit-reproducible.
#include "common.hpp"

namespace {

constexpr int TILE = ISA_SEGSORT_TILE, NT = 256, ROUNDS = TILE / NT, PER_WAVE = TILE / 4;
constexpr uint32_t ONE_BITS = 0x3F800000u, FG_BIT = 0x80000000u;


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

template <int KT>
__device__ __forceinline__ void softmax_row(const float (&l)[KT], float (&p)[KT]) {
    float mx = l[0];
#pragma unroll
    for (int c = 1; c < KT; ++c) mx = fmaxf(mx, l[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < KT; ++c) { p[c] = expf(l[c] - mx); s += p[c]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < KT; ++c) p[c] *= inv;
}


// classes [c0, c0 + nc): keys / vals [nc][B][L], G [nc * (per_image ? B : 1)] (zeroed by the caller).  Grid (x, B).
template <typename T, int KT>
__global__ __launch_bounds__(NT) void lovasz_keys_kernel(View x, const uint8_t* __restrict__ labels, int c0, int nc,
                                                         int per_image, uint32_t* __restrict__ keys,
                                                         uint32_t* __restrict__ vals, int32_t* G) {
    __shared__ int gc[KT];
    const int b = blockIdx.y, K = x.c, B = x.n;
    const long L = (long)x.h * x.w;
    if (threadIdx.x < KT) gc[threadIdx.x] = 0;
    __syncthreads();
    for (long p = (long)blockIdx.x * NT + threadIdx.x; p < L; p += (long)gridDim.x * NT) {
        float l[KT], pr[KT];
        load_row<T, KT>(reinterpret_cast<const T*>(x.data) + ((long)b * L + p) * x.ld, K, l);
        const int y = labels[(long)b * L + p];
        softmax_row<KT>(l, pr);
        const uint32_t idx = (uint32_t)(per_image ? p : (long)b * L + p);
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            if (c >= c0 && c < c0 + nc) {
                const bool fg = c == y;
                float e = fabsf((fg ? 1.f : 0.f) - pr[c]);
                e = fminf(fmaxf(e, 0.f), 1.f);            // NaN -> 0: every key stays inside [0, 0x3F800000]
                const long o = ((long)(c - c0) * B + b) * L + p;
                keys[o] = ONE_BITS - __float_as_uint(e);
                vals[o] = idx | (fg ? FG_BIT : 0u);
            }
        }
        if (y >= c0 && y < c0 + nc) atomicAdd(&gc[y], 1);
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= c0 && c < c0 + nc && c < KT && gc[c] != 0) atomicAdd(G + (per_image ? (long)(c - c0) * B + b : (long)(c - c0)), gc[c]);
}

// foreground count of every tile of the sorted order
__global__ __launch_bounds__(NT) void lovasz_tilecount_kernel(const uint32_t* __restrict__ vals, long seglen, int ntiles,
                                                              uint32_t* __restrict__ cnt) {
    __shared__ int sh[4];
    const int seg = blockIdx.x / ntiles, tile = blockIdx.x - seg * ntiles;
    const uint32_t* v = vals + (long)seg * seglen;
    int n = 0;
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const long i = (long)tile * TILE + j * NT + threadIdx.x;
        if (i < seglen) n += v[i] >> 31;
    }
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = (uint32_t)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// cnt: scanned (foreground pixels of the segment before the tile).  partial [nseg][ntiles]; gpix [nseg][seglen] or NULL.
__global__ __launch_bounds__(NT) void lovasz_apply_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                          const int32_t* __restrict__ G, const uint32_t* __restrict__ cnt,
                                                          long seglen, int ntiles, double* __restrict__ partial,
                                                          float* __restrict__ gpix) {
    __shared__ int wtot[4];
    __shared__ double wsum[4];
    const int seg = blockIdx.x / ntiles, tile = blockIdx.x - seg * ntiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long sbase = (long)seg * seglen, wbase = (long)tile * TILE + wave * PER_WAVE;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t k[ROUNDS], v[ROUNDS];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const long i = wbase + j * 64 + lane;
        const bool valid = i < seglen;
        k[j] = valid ? keys[sbase + i] : ONE_BITS;
        v[j] = valid ? vals[sbase + i] : 0u;
        mine += (int)__popcll(__ballot(v[j] >> 31));
    }
    if (lane == 0) wtot[wave] = mine;
    __syncthreads();
    long run = cnt[blockIdx.x];
    for (int w = 0; w < wave; ++w) run += wtot[w];
    const long Gs = G[seg];
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const long r = wbase + j * 64 + lane;
        const bool fg = v[j] >> 31;
        const uint64_t m = __ballot(fg);
        if (r < seglen) {
            const long cf = run + (long)__popcll(m & below), cb = r - cf;
            const long I = Gs - cf, U = Gs + cb;
            double g;
            if (Gs == 0) g = r == 0 ? 1.0 : 0.0;
            else g = fg ? 1.0 / (double)U : (double)I / ((double)U * (double)(U + 1));
            const uint32_t kb = k[j] <= ONE_BITS ? k[j] : ONE_BITS;
            acc += (double)__uint_as_float(ONE_BITS - kb) * g;
            const long idx = v[j] & ~FG_BIT;
            if (gpix && idx < seglen) gpix[sbase + idx] = (float)(fg ? -g : g);
        }
        run += (long)__popcll(m);
    }
    acc = wave_sum(acc);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// One workgroup.  seg = c * nimg + s (nimg = per_image ? B : 1).
__global__ __launch_bounds__(1024) void lovasz_assemble_kernel(const double* __restrict__ partial, const int32_t* __restrict__ G,
                                                               const float* __restrict__ cfg, int B, int K, int per_image,
                                                               int ntiles, double* segloss, float* __restrict__ scale,
                                                               float* __restrict__ scal) {
    __shared__ double red[16];
    const bool bg = cfg[2] != 0.f, present = cfg[3] != 0.f;
    const int nimg = per_image ? B : 1, nseg = K * nimg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int seg = wave; seg < nseg; seg += 16) {          // one wave per segment: lanes stride the tiles, fixed fold
        double a = 0.0;
        for (int t = lane; t < ntiles; t += 64) a += partial[(long)seg * ntiles + t];
        a = wave_sum(a);
        if (lane == 0) segloss[seg] = a;
    }
    __syncthreads();                                       // one workgroup: its own global writes are visible after this
    const int c0 = bg ? 0 : 1;
    double tot = 0.0;
    for (int s = threadIdx.x; s < nimg; s += 1024) {
        int kept = 0;
        double sum = 0.0;
        for (int c = c0; c < K; ++c)
            if (!present || G[c * nimg + s] > 0) { ++kept; sum += segloss[c * nimg + s]; }
        const float sc = kept ? 1.f / ((float)kept * (float)nimg) : 0.f;
        for (int c = 0; c < K; ++c) scale[c * nimg + s] = (c >= c0 && (!present || G[c * nimg + s] > 0)) ? sc : 0.f;
        tot += kept ? sum / (double)kept : 0.0;
    }
    tot = wave_sum(tot);
    if (lane == 0) red[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += red[w];
        scal[0] = (float)(t / (double)nimg);
    }
}

template <typename T, int KT>
__global__ __launch_bounds__(NT) void lovasz_grad_kernel(View x, const float* __restrict__ gpix, const float* __restrict__ scale,
                                                         int per_image, View dx, int accumulate) {
    __shared__ float ssc[KT];
    const int b = blockIdx.y, K = x.c, B = x.n;
    const long L = (long)x.h * x.w;
    if (threadIdx.x < KT) {
        const int c = threadIdx.x;
        ssc[c] = c < K ? scale[per_image ? c * B + b : c] : 0.f;
    }
    __syncthreads();
    for (long p = (long)blockIdx.x * NT + threadIdx.x; p < L; p += (long)gridDim.x * NT) {
        float l[KT], pr[KT];
        load_row<T, KT>(reinterpret_cast<const T*>(x.data) + ((long)b * L + p) * x.ld, K, l);
        softmax_row<KT>(l, pr);
        // d_k - sum_j p_j d_j with the d of the likeliest class m taken out first: t_j = d_j - d_m, so the j = m term is
        // exactly 0 and no (1 - p_m) is formed from a rounded p_m.  The plain form loses 6e-8 / (1 - p_m) there, and a
        // class absent from the segment puts its whole weight (g_0 = 1) on the pixel where its p is largest.
        float pm = -1.f, dm = 0.f;
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            const float d = c < K ? gpix[((long)c * B + b) * L + p] * ssc[c] : 0.f;
            l[c] = d;                                                 // reuse l[] for d
            if (c < K && pr[c] > pm) { pm = pr[c]; dm = d; }
        }
        float sv = 0.f;
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            l[c] = c < K ? l[c] - dm : 0.f;
            sv += pr[c] * l[c];
        }
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
                o[i] = pr[c] * (l[c] - sv);
                if (accumulate) o[i] += old[i];
            }
            store8g<T>(d + 8 * j, o, nv);
        }
    }
}

// the logits of isa_sem_loss_k_*: 0 when fine, else the status to return
int logits_status(const isa_tensor* x) {
    if (!x || !x->data || x->n <= 0 || x->n > 65535 || x->h <= 0 || x->w <= 0 || x->c < 2 || x->c > ISA_SEM_MAX_CLASSES || x->ld < x->c ||
        x->ld % 8 || tensor_groups(x) != 1)
        return ISA_EINVAL;
    if ((int64_t)x->n * x->h * x->w * x->c >= (1ll << 31)) return ISA_EINVAL;
    if (x->dtype != ISA_F32 && x->dtype != ISA_BF16) return ISA_EDTYPE;
    if (!aligned(x->data, 16)) return ISA_EALIGN;
    return ISA_OK;
}

bool geometry_ok(int32_t nseg, int64_t seglen) {
    return nseg >= 1 && seglen >= 1 && seglen < (1ll << 31) && (int64_t)nseg * seglen < (1ll << 31);
}

}  // namespace

extern "C" int isa_lovasz_keys(const isa_tensor* logits, const uint8_t* labels, int32_t c0, int32_t nc, int32_t per_image,
                               uint32_t* keys, uint32_t* vals, int32_t* G, void* stream) {
    const int rc = logits_status(logits);
    if (rc != ISA_OK) return rc;
    if (!labels || !keys || !vals || !G || c0 < 0 || nc < 1 || c0 + nc > logits->c) return ISA_EINVAL;
    if (!aligned(keys, 4) || !aligned(vals, 4) || !aligned(G, 4)) return ISA_EALIGN;
    const long L = (long)logits->h * logits->w;
    dim3 grid(grid_cap(cdiv(L, NT), 256), logits->n);
    by_dtype(logits->dtype, [&](auto t) { by_width8(logits->c, [&](auto kt) {
        hipLaunchKernelGGL((lovasz_keys_kernel<decltype(t), decltype(kt)::value>), grid, dim3(NT), 0, as_stream(stream),
                           mkview(logits), labels, c0, nc, per_image != 0, keys, vals, G);
    }); });
    return launch_status();
}

extern "C" int isa_lovasz_coef(const uint32_t* keys_sorted, const uint32_t* vals_sorted, const int32_t* G, int32_t nseg,
                               int64_t seglen, uint32_t* tile_counts, double* partial, float* gpix, void* stream) {
    if (!keys_sorted || !vals_sorted || !G || !tile_counts || !partial || !geometry_ok(nseg, seglen)) return ISA_EINVAL;
    if (!aligned(keys_sorted, 4) || !aligned(vals_sorted, 4) || !aligned(G, 4) || !aligned(tile_counts, 4) ||
        !aligned(partial, 8) || !aligned(gpix, 4))
        return ISA_EALIGN;
    const int ntiles = (int)((seglen + TILE - 1) / TILE);
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)(nseg * ntiles));
    hipLaunchKernelGGL(lovasz_tilecount_kernel, grid, dim3(NT), 0, st, vals_sorted, (long)seglen, ntiles, tile_counts);
    if (seg_exclusive_scan_u32(tile_counts, nseg, ntiles, st) != ISA_OK) return ISA_ELAUNCH;
    hipLaunchKernelGGL(lovasz_apply_kernel, grid, dim3(NT), 0, st, keys_sorted, vals_sorted, G, (const uint32_t*)tile_counts,
                       (long)seglen, ntiles, partial, gpix);
    return launch_status();
}

extern "C" int isa_lovasz_assemble(const double* partial, const int32_t* G, const float* cfg, int32_t B, int32_t K,
                                   int32_t per_image, int64_t hw, double* segloss, float* scale, float* scal, void* stream) {
    if (!partial || !G || !cfg || !segloss || !scale || !scal || B <= 0 || K < 2 || K > ISA_SEM_MAX_CLASSES || hw < 1)
        return ISA_EINVAL;
    const int64_t seglen = per_image ? hw : hw * B;
    if (!geometry_ok(K * (per_image ? B : 1), seglen)) return ISA_EINVAL;
    if (!aligned(partial, 8) || !aligned(G, 4) || !aligned(cfg, 4) || !aligned(segloss, 8) || !aligned(scale, 4) ||
        !aligned(scal, 4))
        return ISA_EALIGN;
    const int ntiles = (int)((seglen + TILE - 1) / TILE);
    hipLaunchKernelGGL(lovasz_assemble_kernel, dim3(1), dim3(1024), 0, as_stream(stream), partial, G, cfg, (int)B, (int)K,
                       per_image != 0, ntiles, segloss, scale, scal);
    return launch_status();
}

extern "C" int isa_lovasz_grad(const isa_tensor* logits, const float* gpix, const float* scale, int32_t per_image,
                               const isa_tensor* dlogits, int32_t accumulate, void* stream) {
    int rc = logits_status(logits);
    if (rc != ISA_OK) return rc;
    if (!gpix || !scale || !dlogits || !dlogits->data) return ISA_EINVAL;
    if (!same_shape(dlogits, logits) || dlogits->ld < dlogits->c || dlogits->ld % 8 || tensor_groups(dlogits) != 1) return ISA_EINVAL;
    if (!aligned(dlogits->data, 16) || !aligned(gpix, 4) || !aligned(scale, 4)) return ISA_EALIGN;
    const long L = (long)logits->h * logits->w;
    dim3 grid(grid_cap(cdiv(L, NT), 256), logits->n);
    by_dtype(logits->dtype, [&](auto t) { by_width8(logits->c, [&](auto kt) {
        hipLaunchKernelGGL((lovasz_grad_kernel<decltype(t), decltype(kt)::value>), grid, dim3(NT), 0, as_stream(stream),
                           mkview(logits), gpix, scale, per_image != 0, mkview(dlogits), accumulate);
    }); });
    return launch_status();
}
