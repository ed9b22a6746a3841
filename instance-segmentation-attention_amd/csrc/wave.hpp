// Wave and workgroup collectives of the gfx950 kernel library, each defined once (device only; common.hpp includes this).
// A wave is 64 lanes.  Every function here is called by ALL threads of the wave (wave_*) or of the workgroup (block_*):
// none of them may sit in a divergent branch, and a loop around a block_* call needs a workgroup-uniform bound.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

// ---- wave reductions: xor butterfly, o = 32 ... 1 -------------------------------------------------------------------
// a + b == b + a (and max, min likewise): the two lanes of every exchange compute the same value, so every lane ends with
// the same bits, floating point included.  cluster.hip relies on it: all lanes of a wave take the same branch on a sum.
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
    static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value || std::is_same<T, int>::value ||
                  std::is_same<T, uint32_t>::value || std::is_same<T, unsigned long long>::value,
                  "wave_sum: float, double, int, uint32_t, unsigned long long");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
    return v;
}

// inclusive scan over the lanes of the wave (lane = threadIdx.x % 64: one-dimensional workgroups only); int or uint32_t
template <typename T> __device__ __forceinline__ T wave_incl_scan(T v) {
    static_assert(std::is_same<T, int>::value || std::is_same<T, uint32_t>::value, "wave_incl_scan: int, uint32_t");
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// ---- workgroup collectives ---------------------------------------------------------------------------------------------
// One barrier contract for all of them.  sh holds one T per wave of the workgroup.  A call is
//     barrier;  one lane of each wave writes sh[wave];  barrier;  every thread reads sh
// and returns WITHOUT a trailing barrier.  So: on entry sh may still be in use by the call before (any of these functions,
// on the same sh, back to back or in a loop, is safe); on return other threads may still be reading sh, and a caller that
// writes sh ITSELF afterwards puts a __syncthreads() first.  The leading barrier also publishes what the caller wrote to
// LDS or memory before the call.  Two barriers per call.
//
// block_sum / block_max: the wave results are folded in ascending wave order by every thread, so all threads return the
// same bits and a float or double sum has one fixed order.
template <typename T> __device__ __forceinline__ T block_sum(T v, T* sh) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    T r = 0;
    for (int i = 0; i < nw; ++i) r += sh[i];
    return r;
}
__device__ __forceinline__ float block_max(float v, float* sh) {
    v = wave_max(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    float r = -INFINITY;
    for (int i = 0; i < nw; ++i) r = fmaxf(r, sh[i]);
    return r;
}

// exclusive scan of v over the NT threads of the workgroup in thread order; total: their sum, in every thread.  sh: NT / 64.
template <int NT, typename T> __device__ __forceinline__ T block_excl_scan(T v, T* sh, T& total) {
    static_assert(NT % 64 == 0, "whole waves");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const T incl = wave_incl_scan(v);
    __syncthreads();
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
        const T t = sh[k];
        if (k < wave) before += t;
        total += t;
    }
    return before + incl - v;
}

// In-place exclusive scan of the n entries t[0], t[stride], t[2 stride], ... by the whole workgroup, NT entries a trip with
// a running carry; returns their sum (in every thread).  n is workgroup-uniform, so the trip loop is.
template <int NT, typename T> __device__ __forceinline__ T block_scan_walk(T* t, long n, int stride, T* sh) {
    T carry = 0;
    for (long base = 0; base < n; base += NT) {
        const long i = base + threadIdx.x;
        const T v = i < n ? t[i * stride] : (T)0;
        T total;
        const T ex = block_excl_scan<NT>(v, sh, total);
        if (i < n) t[i * stride] = carry + ex;
        carry += total;
    }
    return carry;
}
