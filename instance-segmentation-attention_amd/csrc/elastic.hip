// Elastic deformation (Simard, Steinkraus & Platt 2003): a smooth random displacement field and the warp of uint8 tensors by
// any displacement field.
//   isa_elastic_field : noise fp32 [n,h,w,2] in [-1,1) -> disp[b,y,x,k] = alpha[b] * G(noise)[b,y,x,k], G a separable Gaussian
//                       blur (along x, then along y) with zeros outside the image (scipy's mode='constant', cval=0);
//   isa_warp_u8       : dst[b,y,x,:] = src sampled at (x + disp[..,0], y + disp[..,1]), nearest or bilinear, coordinates
//                       clamped to the image (replicate border).
// The field takes two launches; a halo of 64 around a two-dimensional tile does not fit the LDS:
//   1 rows:    one workgroup per image row stages the row's w + 2r float2 in LDS, the halo zeroed; lane x sums the 2r+1
//              products in tap order and writes `scratch`.
//   2 columns: a workgroup owns 64 adjacent columns (every row it reads is one 512-byte run) and EL_TR output rows, 8 per
//              wave.  It slides over the input rows y0-r .. y0+EL_TR+r in chunks of EL_CH rows through one LDS tile; every
//              row of a chunk goes to the (at most 8) output rows of the wave it is a tap of.  Chunks and rows ascend, so
//              every output row adds its taps in tap order; the scale by alpha[b] is the last operation.
// The taps travel by value in the kernel arguments (129 floats): no device copy, no allocation, no synchronisation.  Their
// index is wave-uniform in both passes: scalar loads in the first; the second keeps them in LDS between two runs of zeros,
// so its inner loop has no branch and reads them as broadcasts (with the range test and a scalar load per tap the pass
// took 51 us at [16,256,256], radius 32).  fp32, no atomics, a fixed summation order: two runs give the same bits.
// The warp is integer arithmetic after one rounding (see the header), so it can be checked bit for bit.  Lane mapping:
//   c == 32 (the instance planes, NHWC): a lane per pixel and 16-byte channel group, so every gather is a 16-byte load;
//   c <= 4  (image, semantic map): a lane per pixel;
//   else    : a lane per byte.
// In all three adjacent lanes write adjacent bytes.
#include "common.hpp"

namespace {

constexpr int EL_ROW_THREADS = 256;                  // lanes of a row workgroup at most (fewer when w is smaller)
constexpr int EL_COLS = 64;                          // columns of a column workgroup: one wave across
constexpr int EL_RPT = 8;                            // output rows per wave
constexpr int EL_TR = 4 * EL_RPT;                    // output rows per workgroup (4 waves)
constexpr int EL_CH = 32;                            // input rows per LDS chunk
constexpr int WARP_THREADS = 256;

struct ElTaps { float v[2 * ISA_ELASTIC_MAX_RADIUS + 1]; };

typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at a 4-byte aligned address

// ---- launch 1: the rows ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EL_ROW_THREADS) void elastic_rows_kernel(const float2* noise, int w, int r, ElTaps taps, float2* tmp) {
    __shared__ float2 row[ISA_WARP_MAX_SIDE + 2 * ISA_ELASTIC_MAX_RADIUS];
    const long base = ((long)blockIdx.y * gridDim.x + blockIdx.x) * w;
    for (int i = threadIdx.x; i < w + 2 * r; i += blockDim.x) {
        const int x = i - r;
        row[i] = (x >= 0 && x < w) ? noise[base + x] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    for (int x = threadIdx.x; x < w; x += blockDim.x) {
        float2 acc = make_float2(0.f, 0.f);
        for (int k = 0; k <= 2 * r; ++k) {
            const float t = taps.v[k];
            const float2 v = row[x + k];
            acc.x = fmaf(t, v.x, acc.x);
            acc.y = fmaf(t, v.y, acc.y);
        }
        tmp[base + x] = acc;
    }
}

// ---- launch 2: the columns ---------------------------------------------------------------------------------------------------
// grid (ceil(w / 64), ceil(h / EL_TR), n), 256 lanes; wave v owns output rows y0 + 8 v .. y0 + 8 v + 7 of the 64 columns
__global__ __launch_bounds__(256) void elastic_cols_kernel(const float2* tmp, const float* alpha, int h, int w, int r, ElTaps taps,
                                                           float2* disp) {
    __shared__ float2 tile[EL_CH][EL_COLS];
    __shared__ float tp[2 * ISA_ELASTIC_MAX_RADIUS + 1 + 2 * EL_TR];     // the taps with EL_TR zeros on either side
    for (int i = threadIdx.x; i < 2 * r + 1 + 2 * EL_TR; i += 256) {
        const int k = i - EL_TR;
        tp[i] = (k >= 0 && k <= 2 * r) ? taps.v[k] : 0.f;
    }
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x = blockIdx.x * EL_COLS + lane;
    const int y0 = blockIdx.y * EL_TR;
    const int yb = y0 + wv * EL_RPT;
    const long img = (long)blockIdx.z * h;
    const int lo = max(0, y0 - r), hi = min(h, y0 + EL_TR + r);          // the input rows any output row of the workgroup taps
    float2 acc[EL_RPT];
#pragma unroll
    for (int j = 0; j < EL_RPT; ++j) acc[j] = make_float2(0.f, 0.f);
    for (int c0 = lo; c0 < hi; c0 += EL_CH) {
        __syncthreads();                                                 // the chunk before has been read by every wave
#pragma unroll
        for (int j = 0; j < EL_CH / 4; ++j) {
            const int i = wv * (EL_CH / 4) + j, y = c0 + i;
            tile[i][lane] = (y < hi && x < w) ? tmp[(img + y) * w + x] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        const int rows = min(EL_CH, hi - c0);
        // input row c0 + i is tap c0 + i - (yb + j) + r of the wave's output row j: an index in [-31, 2r + 31], so tq[i - j]
        // lies inside tp and is a zero where the row is no tap of that output (an exact no-op on the sum)
        const float* tq = tp + (c0 - yb + r + EL_TR);
#pragma unroll 4
        for (int i = 0; i < rows; ++i) {
            const float2 v = tile[i][lane];
#pragma unroll
            for (int j = 0; j < EL_RPT; ++j) {
                const float tk = tq[i - j];                              // one address for the wave: an LDS broadcast
                acc[j].x = fmaf(tk, v.x, acc[j].x);
                acc[j].y = fmaf(tk, v.y, acc[j].y);
            }
        }
    }
    if (x >= w) return;
    const float a = alpha[blockIdx.z];
#pragma unroll
    for (int j = 0; j < EL_RPT; ++j) {
        const int y = yb + j;
        if (y < h) disp[(img + y) * w + x] = make_float2(a * acc[j].x, a * acc[j].y);
    }
}

// ---- the warp ----------------------------------------------------------------------------------------------------------------
// a displacement in 1/256 pixel: NaN -> 0, clamp to [-16384, 16384] (the product below is then exact), round half to even
__device__ __forceinline__ int warp_quant(float d) {
    d = d != d ? 0.f : d;
    d = fminf(fmaxf(d, -16384.f), 16384.f);
    return (int)rintf(d * 256.0f);
}

// where pixel (x, y) samples: the four tap offsets (in pixels, inside the image) and the four weights (sum 65536); nearest
// mode has one tap, o[0]
struct WarpTaps { int o[4]; int wt[4]; };
template <int MODE>
__device__ __forceinline__ WarpTaps warp_taps(float2 d, int x, int y, int h, int w) {
    const int qx = x * 256 + warp_quant(d.x), qy = y * 256 + warp_quant(d.y);
    WarpTaps t;
    if constexpr (MODE == ISA_WARP_NEAREST) {
        const int xs = min(max((qx + 128) >> 8, 0), w - 1), ys = min(max((qy + 128) >> 8, 0), h - 1);
        t.o[0] = ys * w + xs;
    } else {
        const int x0 = qx >> 8, y0 = qy >> 8, fx = qx & 255, fy = qy & 255;
        const int xa = min(max(x0, 0), w - 1), xb = min(max(x0 + 1, 0), w - 1);
        const int ya = min(max(y0, 0), h - 1), yb = min(max(y0 + 1, 0), h - 1);
        t.o[0] = ya * w + xa; t.o[1] = ya * w + xb; t.o[2] = yb * w + xa; t.o[3] = yb * w + xb;
        t.wt[0] = (256 - fx) * (256 - fy); t.wt[1] = fx * (256 - fy); t.wt[2] = (256 - fx) * fy; t.wt[3] = fx * fy;
    }
    return t;
}

// c <= 4: a lane per pixel
template <int MODE>
__global__ __launch_bounds__(WARP_THREADS) void warp_pixel_kernel(const uint8_t* src, const float2* disp, long total, int h, int w,
                                                                  int c, uint8_t* dst) {
    const int hw = h * w;
    for (long p = (long)blockIdx.x * WARP_THREADS + threadIdx.x; p < total; p += (long)gridDim.x * WARP_THREADS) {
        const int rem = (int)(p % hw);
        const uint8_t* s = src + (p - rem) * c;
        const WarpTaps t = warp_taps<MODE>(disp[p], rem % w, rem / w, h, w);
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (ch >= c) break;
            int v;
            if constexpr (MODE == ISA_WARP_NEAREST) {
                v = s[(long)t.o[0] * c + ch];
            } else {
                v = 32768;
#pragma unroll
                for (int k = 0; k < 4; ++k) v += t.wt[k] * (int)s[(long)t.o[k] * c + ch];
                v >>= 16;
            }
            dst[p * c + ch] = (uint8_t)v;
        }
    }
}

// c == 32: a lane per pixel and 16-byte channel group
template <int MODE>
__global__ __launch_bounds__(WARP_THREADS) void warp_c32_kernel(const uint8_t* src, const float2* disp, long total, int h, int w,
                                                                uint8_t* dst) {
    const int hw = h * w;
    for (long i = (long)blockIdx.x * WARP_THREADS + threadIdx.x; i < total * 2; i += (long)gridDim.x * WARP_THREADS) {
        const long p = i >> 1;
        const int g = (int)(i & 1), rem = (int)(p % hw);
        const uint8_t* s = src + (p - rem) * 32 + g * 16;
        const WarpTaps t = warp_taps<MODE>(disp[p], rem % w, rem / w, h, w);
        u32x4u out;
        if constexpr (MODE == ISA_WARP_NEAREST) {
            out = *reinterpret_cast<const u32x4u*>(s + (long)t.o[0] * 32);
        } else {
            u32x4u a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = *reinterpret_cast<const u32x4u*>(s + (long)t.o[k] * 32);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t word = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    int v = 32768;
#pragma unroll
                    for (int k = 0; k < 4; ++k) v += t.wt[k] * (int)((a[k][q] >> (8 * b)) & 0xffu);
                    word |= (uint32_t)(v >> 16) << (8 * b);
                }
                out[q] = word;
            }
        }
        *reinterpret_cast<u32x4u*>(dst + i * 16) = out;
    }
}

// any other c: a lane per byte
template <int MODE>
__global__ __launch_bounds__(WARP_THREADS) void warp_byte_kernel(const uint8_t* src, const float2* disp, long total, int h, int w,
                                                                 int c, uint8_t* dst) {
    const int hw = h * w;
    for (long i = (long)blockIdx.x * WARP_THREADS + threadIdx.x; i < total * c; i += (long)gridDim.x * WARP_THREADS) {
        const long p = i / c;
        const int ch = (int)(i - p * c), rem = (int)(p % hw);
        const uint8_t* s = src + (p - rem) * c + ch;
        const WarpTaps t = warp_taps<MODE>(disp[p], rem % w, rem / w, h, w);
        int v;
        if constexpr (MODE == ISA_WARP_NEAREST) {
            v = s[(long)t.o[0] * c];
        } else {
            v = 32768;
#pragma unroll
            for (int k = 0; k < 4; ++k) v += t.wt[k] * (int)s[(long)t.o[k] * c];
            v >>= 16;
        }
        dst[i] = (uint8_t)v;
    }
}

// workgroups for `items` lanes of a grid-stride walk (n*h*w*c does not fit an int)
int warp_grid(long items) { return grid_cap((items + WARP_THREADS - 1) / WARP_THREADS); }

template <int MODE>
void warp_launch(const uint8_t* src, const float2* disp, long total, int h, int w, int c, uint8_t* dst, hipStream_t st) {
    if (c == 32)
        hipLaunchKernelGGL(warp_c32_kernel<MODE>, dim3(warp_grid(total * 2)), dim3(WARP_THREADS), 0, st, src, disp,
                           total, h, w, dst);
    else if (c <= 4)
        hipLaunchKernelGGL(warp_pixel_kernel<MODE>, dim3(warp_grid(total)), dim3(WARP_THREADS), 0, st, src, disp,
                           total, h, w, c, dst);
    else
        hipLaunchKernelGGL(warp_byte_kernel<MODE>, dim3(warp_grid(total * c)), dim3(WARP_THREADS), 0, st, src, disp,
                           total, h, w, c, dst);
}

bool el_shape_ok(int32_t n, int32_t h, int32_t w) {
    return n >= 1 && n <= 65535 && h >= 1 && h <= ISA_WARP_MAX_SIDE && w >= 1 && w <= ISA_WARP_MAX_SIDE;
}

}  // namespace

extern "C" int isa_elastic_field(const float* noise, const float* alpha_dev, int32_t n, int32_t h, int32_t w,
                                 const float* taps_host, int32_t radius, float* disp, void* scratch, int64_t scratch_bytes,
                                 void* stream) {
    if (!noise || !alpha_dev || !taps_host || !disp || !scratch || !el_shape_ok(n, h, w) || radius < 0 ||
        radius > ISA_ELASTIC_MAX_RADIUS)
        return ISA_EINVAL;
    const uintptr_t bytes = (uintptr_t)ISA_ELASTIC_SCRATCH_BYTES(n, h, w);      // of noise, disp and the scratch alike
    if (ranges_overlap(disp, bytes, noise, bytes) || ranges_overlap(scratch, bytes, noise, bytes) ||
        ranges_overlap(scratch, bytes, disp, bytes))
        return ISA_EINVAL;
    if (!aligned(noise, 8) || !aligned(disp, 8) || !aligned(alpha_dev, 4) || !aligned(scratch, 16)) return ISA_EALIGN;
    if (scratch_bytes < ISA_ELASTIC_SCRATCH_BYTES(n, h, w)) return ISA_ENOMEM;
    ElTaps taps = {};
    if (radius == 0) taps.v[0] = 1.f;                                           // disp = alpha * noise, whatever the one tap says
    else for (int k = 0; k <= 2 * radius; ++k) taps.v[k] = taps_host[k];
    float2* tmp = reinterpret_cast<float2*>(scratch);
    hipStream_t st = as_stream(stream);
    const int lanes = min(EL_ROW_THREADS, cdiv(w, 64) * 64);
    hipLaunchKernelGGL(elastic_rows_kernel, dim3(h, n), dim3(lanes), 0, st, reinterpret_cast<const float2*>(noise), w, radius, taps,
                       tmp);
    hipLaunchKernelGGL(elastic_cols_kernel, dim3(cdiv(w, EL_COLS), cdiv(h, EL_TR), n), dim3(256), 0, st, tmp, alpha_dev, h, w, radius,
                       taps, reinterpret_cast<float2*>(disp));
    return launch_status();
}

extern "C" int isa_warp_u8(const uint8_t* src, const float* disp, int32_t n, int32_t h, int32_t w, int32_t c, int32_t mode,
                           uint8_t* dst, void* stream) {
    if (!src || !disp || !dst || !el_shape_ok(n, h, w) || c < 1 || c > ISA_WARP_MAX_CHANNELS ||
        (mode != ISA_WARP_NEAREST && mode != ISA_WARP_BILINEAR))
        return ISA_EINVAL;
    const long total = (long)n * h * w;
    if (ranges_overlap(dst, (uintptr_t)total * c, src, (uintptr_t)total * c)) return ISA_EINVAL;
    if (ranges_overlap(dst, (uintptr_t)total * c, disp, (uintptr_t)total * 8)) return ISA_EINVAL;
    if (!aligned(disp, 8) || !aligned(src, 4) || !aligned(dst, 4)) return ISA_EALIGN;
    const float2* d = reinterpret_cast<const float2*>(disp);
    if (mode == ISA_WARP_NEAREST) warp_launch<ISA_WARP_NEAREST>(src, d, total, h, w, c, dst, as_stream(stream));
    else warp_launch<ISA_WARP_BILINEAR>(src, d, total, h, w, c, dst, as_stream(stream));
    return launch_status();
}
