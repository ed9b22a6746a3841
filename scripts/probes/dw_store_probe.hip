// Store pattern of the depthwise kernels (dwconv.hip): a workgroup owns an 8 x 32-pixel tile x 32 channels; lane =
// (cg = tid & 3: 8 channels, g = tid >> 2: tile row g >> 3, four consecutive x at (g & 7) * 4) and stores its four pixels with
// four 16-byte stores.  With C = 64 channels a pixel row is one 128-byte line and the two channel blocks (blockIdx.y) write
// its two halves from different workgroups.  Variants (write-only and read + write, 1 GiB tensors):
//   A  the kernel's mapping, channel block 32 of C = 64            (half lines per workgroup)
//   B  the same lanes but a workgroup covers all 64 channels of a 8 x 16-pixel tile (whole lines per store instruction group)
//   C  contiguous 16 bytes per lane (upper bound)
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int MODE, bool READ>
__global__ __launch_bounds__(256) void k(const char* in, char* out, int n, int h, int w, int C, float* sink) {
    const int tid = threadIdx.x;
    f32x4 acc = {1, 2, 3, 4};
    if (MODE == 2) {
        const long total = (long)n * h * w * C * 2 / 16;
        for (long i = (long)blockIdx.x * 256 + tid; i < total; i += (long)gridDim.x * 256) {
            if (READ) acc += *reinterpret_cast<const f32x4*>(in + i * 16);
            *reinterpret_cast<f32x4*>(out + i * 16) = acc;
        }
    } else if (MODE == 0) {
        const int cg = tid & 3, g = tid >> 2, row = g >> 3, x0 = (g & 7) * 4;
        const int tiles_x = w / 32, tiles_y = h / 8; const long ntiles = (long)n * tiles_x * tiles_y;
        const int cb = blockIdx.y;
        for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
            const int tx = (int)(t % tiles_x); const long q = t / tiles_x; const int ty = (int)(q % tiles_y); const int b = (int)(q / tiles_y);
            const long base = ((((long)b * h + ty * 8 + row) * w + tx * 32 + x0) * C + cb * 32 + cg * 8) * 2;
            for (int o = 0; o < 4; ++o) {
                if (READ) acc += *reinterpret_cast<const f32x4*>(in + base + (long)o * C * 2);
                *reinterpret_cast<f32x4*>(out + base + (long)o * C * 2) = acc;
            }
        }
    } else {   // MODE 1: 8 lanes per pixel (64 channels), tile 8 x 16 pixels, four consecutive x per lane
        const int cg = tid & 7, g = tid >> 3, row = g >> 2, x0 = (g & 3) * 4;
        const int tiles_x = w / 16, tiles_y = h / 8; const long ntiles = (long)n * tiles_x * tiles_y;
        for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
            const int tx = (int)(t % tiles_x); const long q = t / tiles_x; const int ty = (int)(q % tiles_y); const int b = (int)(q / tiles_y);
            const long base = ((((long)b * h + ty * 8 + row) * w + tx * 16 + x0) * C + cg * 8) * 2;
            for (int o = 0; o < 4; ++o) {
                if (READ) acc += *reinterpret_cast<const f32x4*>(in + base + (long)o * C * 2);
                *reinterpret_cast<f32x4*>(out + base + (long)o * C * 2) = acc;
            }
        }
    }
    if (acc[0] == 12345.f) sink[0] = acc[1];
}

template <int MODE, bool READ>
float run(const char* in, char* out, int n, int h, int w, int C, float* sink, dim3 grid) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    float best = 1e9f;
    for (int rep = 0; rep < 4; ++rep) {
        hipEventRecord(e0);
        hipLaunchKernelGGL((k<MODE, READ>), grid, dim3(256), 0, 0, in, out, n, h, w, C, sink);
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1); if (ms < best) best = ms;
    }
    return best;
}

int main() {
    const int n = 128, h = 256, w = 256, C = 64;                    // 1 GiB per tensor in bf16
    const double bytes = (double)n * h * w * C * 2;
    char *in, *out; float* sink;
    hipMalloc(&in, (size_t)bytes); hipMalloc(&out, (size_t)bytes); hipMalloc(&sink, 4);
    hipMemset(in, 0, (size_t)bytes);
    printf("write only:   A (32-channel blocks, half lines) %.0f GB/s   B (64 channels per workgroup, whole lines) %.0f GB/s   C contiguous %.0f GB/s\n",
           bytes / run<0, false>(in, out, n, h, w, C, sink, dim3(128, 2)) / 1e6, bytes / run<1, false>(in, out, n, h, w, C, sink, dim3(256)) / 1e6,
           bytes / run<2, false>(in, out, n, h, w, C, sink, dim3(2048)) / 1e6);
    printf("read + write: A %.0f GB/s   B %.0f GB/s   C %.0f GB/s   (bytes read + written)\n",
           2 * bytes / run<0, true>(in, out, n, h, w, C, sink, dim3(128, 2)) / 1e6, 2 * bytes / run<1, true>(in, out, n, h, w, C, sink, dim3(256)) / 1e6,
           2 * bytes / run<2, true>(in, out, n, h, w, C, sink, dim3(2048)) / 1e6);
    printf("more workgroups (A: 384 x 2, B: 768):  read + write A %.0f GB/s   B %.0f GB/s\n",
           2 * bytes / run<0, true>(in, out, n, h, w, C, sink, dim3(384, 2)) / 1e6, 2 * bytes / run<1, true>(in, out, n, h, w, C, sink, dim3(768)) / 1e6);
    return 0;
}
