// The pixel-by-pixel augmentations of AlignCollate.__preprocess (code/lib/dataset.py:271-281) in one pass on the device:
// colour jitter (dataset.py:147-149 -> utils.py:58-59 -> torchvision ColorJitter: ImageEnhance.Brightness / Contrast /
// Color and the HSV hue shift of adjust_hue's PIL path, in a drawn order), gamma (dataset.py:154-155 ->
// preprocess.py:405-439: Image.point over a float table), channel swap (dataset.py:152-153 -> preprocess.py:381-401)
// and grayscale (dataset.py:150-151 -> utils.py:62-63 -> RandomGrayscale: convert('L') to three channels).  The reference
// makes up to seven PIL passes over the image on the host; here a pixel is read once, goes through its image's program
// (isa_photo_prog: jitter ops in order -> LUT -> channel map -> grayscale) in registers, and is written once.  Every
// stage rounds to uint8 exactly where Pillow holds a uint8 image, so the result is bit-identical to the installed
// Pillow: tests/photometric_np.py restates the arithmetic below and tests/test_photometric_ref.py pins it.
// At the loader's sizes (one image of 0.1-5 MB per call) the call is launch-latency bound: what the fusion saves is
// launches as much as bytes.
#include "common.hpp"

namespace {

static_assert(sizeof(isa_photo_prog) == 288, "isa_photo_prog is mirrored field by field in lib.py");

// ---- pixel arithmetic ----------------------------------------------------------------------------------------------
// Floating-point contraction is off throughout: Pillow's x86-64 build rounds after every operation.

// convert('L'): ITU-R 601-2 luma in 16-bit fixed point
__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(degenerate d, image x, f), libImaging/Blend.c: float32 d + f * (x - d); truncated for 0 <= f <= 1, else
// clipped to [0, 255] and truncated.  For 0 <= f <= 1 the value lies in [0, 255] already, so the clip serves both.
__device__ __forceinline__ int blend(int x, int d, float f) {
#pragma clang fp contract(off)
    const float t = (float)d + f * (float)(x - d);
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// convert('HSV'), libImaging/Convert.c rgb2hsv_row: the quotients are float32; the hue sums mix in double literals, so
// they are formed in double and stored to float32; so is fmod(h / 6.0 + 1.0, 1.0); the byte is (int)(h * 255.0) in
// double.  One precision throughout gets tens of thousands of the 2^24 colours' hues wrong.
__device__ __forceinline__ void rgb2hsv(int r, int g, int b, int& uh, int& us, int& uv) {
#pragma clang fp contract(off)
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    uv = maxc;
    if (minc == maxc) { uh = 0; us = 0; return; }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = (float)((double)bc - (double)gc);
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double t = (double)h / 6.0 + 1.0;              // in (0.8, 1.9)
    h = (float)(t - floor(t));                           // fmod(t, 1.0), exact
    uh = min(max((int)((double)h * 255.0), 0), 255);
    us = min(max((int)((double)s * 255.0), 0), 255);
}

// C round() of a non-negative float: half up
__device__ __forceinline__ int round_half_up(float x) {
    const float fl = floorf(x);
    return (int)fl + (x - fl >= 0.5f ? 1 : 0);
}

// convert('RGB') of an HSV image, Convert.c hsv2rgb: float32 throughout, the three products rounded half up
__device__ __forceinline__ void hsv2rgb(int h, int s, int v, int& r, int& g, int& b) {
#pragma clang fp contract(off)
    if (s == 0) { r = g = b = v; return; }
    const float hf = (float)h * 6.0f / 255.0f;
    const float fi = floorf(hf);
    const float f = hf - fi;
    const float fs = (float)s / 255.0f, fv = (float)v;
    const int p = min(max(round_half_up(fv * (1.0f - fs)), 0), 255);
    const int q = min(max(round_half_up(fv * (1.0f - fs * f)), 0), 255);
    const int t = min(max(round_half_up(fv * (1.0f - fs * (1.0f - f))), 0), 255);
    switch ((int)fi % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// ---- programs ------------------------------------------------------------------------------------------------------
// One image's program as the kernels use it: wave-uniform values (an image is a blockIdx.y), so they sit in SGPRs.
struct Ctl {
    int n_ops, op[4]; float f[4];
    int shift, use_lut, gray, chan[3];
    int m;                       // contrast's degenerate: int(mean(L) + 0.5)
    int contrast_at;             // index of the contrast op, n_ops when there is none (or no workspace to take m from)
};

__device__ __forceinline__ Ctl load_ctl(const isa_photo_prog* p, bool have_sums) {
    Ctl c;
    c.n_ops = min(max(p->n_ops, 0), 4);
    c.contrast_at = c.n_ops;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c.op[k] = k < c.n_ops ? p->op[k] : -1;
        c.f[k] = p->factor[k];
        if (c.op[k] == ISA_PHOTO_CONTRAST) {
            if (have_sums && c.contrast_at == c.n_ops) c.contrast_at = k;
            if (!have_sums) c.op[k] = -1;                // no workspace, no mean: the op is skipped, never a null read
        }
    }
    c.shift = p->hue_shift; c.use_lut = p->use_lut; c.gray = p->gray;
#pragma unroll
    for (int k = 0; k < 3; ++k) c.chan[k] = min((int)p->chan[k], 2);
    c.m = 0;
    return c;
}

// Jitter ops [0, upto) on N pixels held in registers.  The op loop is the outer one: its switch is wave-uniform, and
// each case is straight-line code over the N pixels.
template <int N>
__device__ __forceinline__ void jitter(int (&r)[N], int (&g)[N], int (&b)[N], const Ctl& c, int upto) {
    for (int k = 0; k < upto; ++k) {
        const float f = k == 0 ? c.f[0] : (k == 1 ? c.f[1] : (k == 2 ? c.f[2] : c.f[3]));       // selects, not an indexed array
        switch (k == 0 ? c.op[0] : (k == 1 ? c.op[1] : (k == 2 ? c.op[2] : c.op[3]))) {
            case ISA_PHOTO_BRIGHTNESS:
#pragma unroll
                for (int i = 0; i < N; ++i) { r[i] = blend(r[i], 0, f); g[i] = blend(g[i], 0, f); b[i] = blend(b[i], 0, f); }
                break;
            case ISA_PHOTO_CONTRAST:
#pragma unroll
                for (int i = 0; i < N; ++i) { r[i] = blend(r[i], c.m, f); g[i] = blend(g[i], c.m, f); b[i] = blend(b[i], c.m, f); }
                break;
            case ISA_PHOTO_SATURATION:
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const int l = luma(r[i], g[i], b[i]);
                    r[i] = blend(r[i], l, f); g[i] = blend(g[i], l, f); b[i] = blend(b[i], l, f);
                }
                break;
            case ISA_PHOTO_HUE:
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    int h, s, v;
                    rgb2hsv(r[i], g[i], b[i], h, s, v);
                    hsv2rgb((h + c.shift) & 255, s, v, r[i], g[i], b[i]);
                }
                break;
            default: break;
        }
    }
}

// The whole program on N pixels: jitter -> LUT (a 256-byte copy in LDS) -> channel map -> grayscale
template <int N>
__device__ __forceinline__ void run_program(int (&r)[N], int (&g)[N], int (&b)[N], const Ctl& c, const uint8_t* lut) {
    jitter<N>(r, g, b, c, c.n_ops);
    if (c.use_lut) {
#pragma unroll
        for (int i = 0; i < N; ++i) { r[i] = lut[r[i]]; g[i] = lut[g[i]]; b[i] = lut[b[i]]; }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int v[3] = {r[i], g[i], b[i]};
        int o[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = c.chan[k] == 0 ? v[0] : (c.chan[k] == 1 ? v[1] : v[2]);
        if (c.gray) o[0] = o[1] = o[2] = luma(o[0], o[1], o[2]);
        r[i] = o[0]; g[i] = o[1]; b[i] = o[2];
    }
}

// Contrast's mean is that of Pillow's int(ImageStat.Stat(L).mean[0] + 0.5): a Python float sum / count, plus 0.5,
// truncated.  In integers it is (2 sum + count) / (2 count), the floor of the exact sum / count + 1/2.  The two agree:
// when the exact value is an integer plus a half, the float quotient and the sum with 0.5 are both exact; otherwise it
// is at least 1 / (2 count) > 2^-33 away from one, while the two float roundings move it by less than 2^-44 (the value
// is below 256 and carries 53 bits), so it is never close enough to a half for a rounding to carry it across.
__device__ __forceinline__ int contrast_mean(long sum, long count) { return (int)((2 * sum + count) / (2 * count)); }

// ---- kernels -------------------------------------------------------------------------------------------------------
// Pre-pass: sums[b] += L of every pixel of image b after the jitter ops listed before its contrast op.  One pixel per
// lane; images without a contrast op leave at once.  grid (x, n).
__global__ __launch_bounds__(256) void photo_luma_sum_kernel(const uint8_t* src, long npix, const isa_photo_prog* progs,
                                                             unsigned long long* sums) {
    __shared__ unsigned long long part[4];
    const int b = blockIdx.y;
    const Ctl c = load_ctl(progs + b, true);
    if (c.contrast_at == c.n_ops) return;
    const uint8_t* s = src + (long)b * npix * 3;
    unsigned long long acc = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
        int r[1] = {s[3 * i]}, g[1] = {s[3 * i + 1]}, bl[1] = {s[3 * i + 2]};
        jitter<1>(r, g, bl, c, c.contrast_at);
        acc += (unsigned)luma(r[0], g[0], bl[0]);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + b, part[0] + part[1] + part[2] + part[3]);
}

// The pass.  grid (x, n): image b starts at byte b * npix * 3, in general not a multiple of 16, so every image has its
// own split: `head` leading pixels up to the first pixel that starts on a 16-byte boundary (3 * head = -address mod 16,
// head = -address * 11 mod 16 since 3 * 11 = 1 mod 16), then chunks of 16 pixels = 48 bytes = three 16-byte loads and
// stores per lane, then the pixels left over.  Head and leftover pixels go one per lane.  The three loads of a wave
// together cover 3 KB contiguously; each one touches every line of it, the second and third hit what the first
// brought.  vec == 0 (src and dst differ mod 16): every pixel goes the one-per-lane way.
// Sixteen pixels in flight per lane, the hue case above all, cost 187 VGPRs: two waves per SIMD, nothing in scratch.
// Bounding the kernel to 128 registers spills 340 bytes per lane, so it is left alone: a byte stream with three 16-byte
// loads per lane outstanding does not need more waves than that to fill the memory pipeline.
__global__ __launch_bounds__(256) void photometric_kernel(const uint8_t* src, uint8_t* dst, long npix, const isa_photo_prog* progs,
                                                          const long* sums, int vec) {
    __shared__ uint8_t lut[256];
    const int b = blockIdx.y;
    Ctl c = load_ctl(progs + b, sums != nullptr);
    if (c.contrast_at < c.n_ops) c.m = contrast_mean(sums[b], npix);
    lut[threadIdx.x] = progs[b].lut[threadIdx.x];
    __syncthreads();
    const uint8_t* s = src + (long)b * npix * 3;
    uint8_t* d = dst + (long)b * npix * 3;
    long head = npix, chunks = 0;
    if (vec) {
        head = (long)(((16 - (reinterpret_cast<uintptr_t>(s) & 15)) * 11) & 15);
        if (head > npix) head = npix;
        chunks = (npix - head) / 16;
    }
    const long rest0 = head + chunks * 16;                // first leftover pixel
    const long items = chunks + (npix - chunks * 16);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        if (i < chunks) {
            const long off = (head + i * 16) * 3;
            uint32_t w[12];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint4 v = *reinterpret_cast<const uint4*>(s + off + 16 * j);
                w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
            }
            int r[16], g[16], bl[16];
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                r[p] = (w[(3 * p) >> 2] >> (8 * ((3 * p) & 3))) & 255;
                g[p] = (w[(3 * p + 1) >> 2] >> (8 * ((3 * p + 1) & 3))) & 255;
                bl[p] = (w[(3 * p + 2) >> 2] >> (8 * ((3 * p + 2) & 3))) & 255;
            }
            run_program<16>(r, g, bl, c, lut);
#pragma unroll
            for (int j = 0; j < 12; ++j) w[j] = 0;
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                w[(3 * p) >> 2] |= (uint32_t)r[p] << (8 * ((3 * p) & 3));
                w[(3 * p + 1) >> 2] |= (uint32_t)g[p] << (8 * ((3 * p + 1) & 3));
                w[(3 * p + 2) >> 2] |= (uint32_t)bl[p] << (8 * ((3 * p + 2) & 3));
            }
#pragma unroll
            for (int j = 0; j < 3; ++j)
                *reinterpret_cast<uint4*>(d + off + 16 * j) = uint4{w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]};
        } else {
            const long j = i - chunks;                      // head pixels first, then the leftovers
            const long off = (j < head ? j : rest0 + (j - head)) * 3;
            int r[1] = {s[off]}, g[1] = {s[off + 1]}, bl[1] = {s[off + 2]};
            run_program<1>(r, g, bl, c, lut);
            d[off] = (uint8_t)r[0]; d[off + 1] = (uint8_t)g[0]; d[off + 2] = (uint8_t)bl[0];
        }
    }
}

}  // namespace

extern "C" int isa_photometric_u8(const uint8_t* src, uint8_t* dst, int32_t n, int32_t h, int32_t w, const isa_photo_prog* progs_dev,
                                  int32_t has_contrast, int64_t* sums_ws, void* stream) {
    if (!src || !dst || !progs_dev || n <= 0 || n > 65535 || h <= 0 || w <= 0) return ISA_EINVAL;
    if (has_contrast && !sums_ws) return ISA_EINVAL;
    if (has_contrast && !aligned(sums_ws, 8)) return ISA_EALIGN;
    hipStream_t s = as_stream(stream);
    const long npix = (long)h * w;
    const int per_image = 2048 / n > 0 ? 2048 / n : 1;     // about 2048 workgroups in all, grid-stride beyond
    if (has_contrast) {
        if (hipMemsetAsync(sums_ws, 0, (size_t)n * 8, s) != hipSuccess) return ISA_ELAUNCH;
        hipLaunchKernelGGL(photo_luma_sum_kernel, dim3(grid_cap(cdiv(npix, 256), per_image), n), dim3(256), 0, s, src, npix,
                           progs_dev, reinterpret_cast<unsigned long long*>(sums_ws));
    }
    const int vec = ((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    // a lane takes 16 pixels on the vector path
    hipLaunchKernelGGL(photometric_kernel, dim3(grid_cap(cdiv(vec ? npix / 16 + 32 : npix, 256), per_image), n), dim3(256), 0, s,
                       src, dst, npix, progs_dev, has_contrast ? reinterpret_cast<const long*>(sums_ws) : nullptr, vec);
    return launch_status();
}
