// Optimizers on the flat parameter buffer besides Adadelta (head_bwd.hip): torch.optim.Adam, RMSprop and SGD as the
// reference constructs them (model.py:145-166: L2 weight decay added to the gradient, SGD momentum 0.9, library
// defaults otherwise), each fused with the global-norm clip (model.py:273-278) in one streaming pass:
//   gr = g * (gscale * clip) + wd * p ;  state update ;  parameter write
// clip = min(1, max_norm / (sqrt(sqnorm[0]) + 1e-6)) when max_norm > 0 (isa_sqnorm wrote sqnorm), else 1.  It is a
// uniform scalar, computed in double so that its rounding does not reach every element.
// The kernels are memory-bound (Adam 28 B per element, RMSprop and SGD 20 B): 16-byte loads and stores, a grid-stride
// loop over groups of 4 floats on a capped grid, and the last n % 4 elements in scalar code.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int OPT_GRID_CAP = 1024;      // workgroups of 256 threads: 4 per CU, each lane keeps 4-7 16-byte accesses in flight

__device__ __forceinline__ float grad_scale(const float* sqnorm, float max_norm, float gscale) {
    double clip = 1.0;
    if (max_norm > 0.f) clip = fmin(1.0, (double)max_norm / (sqrt((double)sqnorm[0]) + 1e-6));
    return (float)((double)gscale * clip);
}

// torch.optim.Adam (no amsgrad): exp_avg.lerp_(grad, 1 - b1); exp_avg_sq = b2 * exp_avg_sq + (1 - b2) * grad^2;
// p -= lr / (1 - b1^t) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - b2^t) + eps)
struct AdamOp {
    static constexpr int NS = 2;
    const float* aux;                    // written by adam_prepare_kernel: {gscale * clip, 1 - b1^t, 1 - b2^t, sqrt(1 - b2^t)}
    const float* lr_dev;
    float lr, b2, omb1, omb2, eps, wd;
    struct Coef { float gs, step, sbc2; };
    __device__ __forceinline__ Coef coef() const {
        const float l = lr_dev ? lr_dev[0] : lr;
        return Coef{aux[0], l / aux[1], aux[3]};
    }
    __device__ __forceinline__ void apply(const Coef& c, float& w, float g, float& m, float& v) const {
        const float gr = g * c.gs + wd * w;
        m = m + omb1 * (gr - m);
        v = b2 * v + omb2 * gr * gr;
        w = w - c.step * (m / (sqrtf(v) / c.sbc2 + eps));
    }
};

// torch.optim.RMSprop (no momentum, not centred): square_avg = alpha * square_avg + (1 - alpha) * grad^2;
// p -= lr * grad / (sqrt(square_avg) + eps)
struct RmspropOp {
    static constexpr int NS = 1;
    const float* sqnorm;
    const float* lr_dev;
    float lr, alpha, oma, eps, wd, max_norm, gscale;
    struct Coef { float gs, lr; };
    __device__ __forceinline__ Coef coef() const {
        return Coef{grad_scale(sqnorm, max_norm, gscale), lr_dev ? lr_dev[0] : lr};
    }
    __device__ __forceinline__ void apply(const Coef& c, float& w, float g, float& s, float&) const {
        const float gr = g * c.gs + wd * w;
        s = alpha * s + oma * gr * gr;
        w = w - c.lr * (gr / (sqrtf(s) + eps));
    }
};

// torch.optim.SGD (dampening 0, no Nesterov): buf = momentum * buf + grad; p -= lr * buf.  torch copies the gradient
// into the buffer on the first step; a zero-initialised buffer gives the same bits.
struct SgdOp {
    static constexpr int NS = 1;
    const float* sqnorm;
    const float* lr_dev;
    float lr, momentum, wd, max_norm, gscale;
    struct Coef { float gs, lr; };
    __device__ __forceinline__ Coef coef() const {
        return Coef{grad_scale(sqnorm, max_norm, gscale), lr_dev ? lr_dev[0] : lr};
    }
    __device__ __forceinline__ void apply(const Coef& c, float& w, float g, float& b, float&) const {
        const float gr = g * c.gs + wd * w;
        b = momentum * b + gr;
        w = w - c.lr * b;
    }
};

// p, g, s0 (and s1 when Op::NS == 2) are 16-byte aligned ranges of n floats.
template <class Op>
__global__ __launch_bounds__(256) void optim_kernel(float* p, const float* g, float* s0, float* s1, long n, Op op) {
    const typename Op::Coef c = op.coef();
    const long n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* a4 = reinterpret_cast<f32x4*>(s0);
    f32x4* b4 = reinterpret_cast<f32x4*>(s1);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 w = p4[i], a = a4[i], b = {0.f, 0.f, 0.f, 0.f};
        const f32x4 gv = g4[i];
        if constexpr (Op::NS == 2) b = b4[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float wj = w[j], aj = a[j], bj = b[j];
            op.apply(c, wj, gv[j], aj, bj);
            w[j] = wj; a[j] = aj; b[j] = bj;
        }
        a4[i] = a;
        if constexpr (Op::NS == 2) b4[i] = b;
        p4[i] = w;
    }
    const long t = (n4 << 2) + threadIdx.x;          // the last n % 4 elements
    if (blockIdx.x == 0 && t < n) {
        float w = p[t], a = s0[t], b = 0.f;
        if constexpr (Op::NS == 2) b = s1[t];
        op.apply(c, w, g[t], a, b);
        s0[t] = a;
        if constexpr (Op::NS == 2) s1[t] = b;
        p[t] = w;
    }
}

// One thread, ahead of the Adam update on the same stream: advances the step count in device memory (a replayed
// hipGraph repeats its kernel arguments, so a host-side count would freeze the bias correction at its captured value)
// and writes the scalars every workgroup of the update then reads.
__global__ void adam_prepare_kernel(int* step, float* aux, double b1, double b2, const float* sqnorm, float max_norm,
                                    float gscale) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int t = step[0] + 1;
    step[0] = t;
    const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
    aux[0] = grad_scale(sqnorm, max_norm, gscale);
    aux[1] = (float)bc1;
    aux[2] = (float)bc2;
    aux[3] = (float)sqrt(bc2);
}

inline bool finite_f(double v) { return isfinite(v); }
// what every entry shares: lr, weight decay, clip and the averaging scale
inline bool common_ok(float lr, float wd, const float* sqnorm, float max_norm, float gscale) {
    if (!finite_f(lr) || lr < 0.f || !finite_f(wd) || wd < 0.f || !finite_f(max_norm) || !finite_f(gscale)) return false;
    return !(max_norm > 0.f && !sqnorm);
}

template <class Op>
int launch(float* p, const float* g, float* s0, float* s1, int64_t n, const Op& op, void* stream) {
    const int grid = grid_cap(cdiv(n >> 2, 256), OPT_GRID_CAP);
    hipLaunchKernelGGL(optim_kernel<Op>, dim3(grid), dim3(256), 0, as_stream(stream), p, g, s0, s1, (long)n, op);
    return launch_status();
}

}  // namespace

extern "C" int isa_adam(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int32_t* step, float* aux, int64_t n,
                        float lr, double beta1, double beta2, float eps, float wd, const float* sqnorm, float max_norm,
                        float gscale, const float* lr_dev, void* stream) {
    if (!p || !g || !exp_avg || !exp_avg_sq || !step || !aux || n <= 0) return ISA_EINVAL;
    if (!common_ok(lr, wd, sqnorm, max_norm, gscale) || !finite_f(eps) || eps < 0.f) return ISA_EINVAL;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return ISA_EINVAL;
    if (!aligned(p, 16) || !aligned(g, 16) || !aligned(exp_avg, 16) || !aligned(exp_avg_sq, 16) || !aligned(aux, 16))
        return ISA_EALIGN;
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(64), 0, as_stream(stream), step, aux, beta1, beta2, sqnorm,
                       max_norm, gscale);
    const AdamOp op{aux, lr_dev, lr, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd};
    return launch(p, g, exp_avg, exp_avg_sq, n, op, stream);
}

extern "C" int isa_rmsprop(float* p, const float* g, float* square_avg, int64_t n, float lr, double alpha, float eps,
                           float wd, const float* sqnorm, float max_norm, float gscale, const float* lr_dev, void* stream) {
    if (!p || !g || !square_avg || n <= 0) return ISA_EINVAL;
    if (!common_ok(lr, wd, sqnorm, max_norm, gscale) || !finite_f(eps) || eps < 0.f) return ISA_EINVAL;
    if (!(alpha >= 0.0 && alpha <= 1.0)) return ISA_EINVAL;
    if (!aligned(p, 16) || !aligned(g, 16) || !aligned(square_avg, 16)) return ISA_EALIGN;
    const RmspropOp op{sqnorm, lr_dev, lr, (float)alpha, (float)(1.0 - alpha), eps, wd, max_norm, gscale};
    return launch(p, g, square_avg, nullptr, n, op, stream);
}

extern "C" int isa_sgd(float* p, const float* g, float* momentum_buffer, int64_t n, float lr, double momentum, float wd,
                       const float* sqnorm, float max_norm, float gscale, const float* lr_dev, void* stream) {
    if (!p || !g || !momentum_buffer || n <= 0) return ISA_EINVAL;
    if (!common_ok(lr, wd, sqnorm, max_norm, gscale)) return ISA_EINVAL;
    if (!(momentum >= 0.0) || !finite_f(momentum)) return ISA_EINVAL;
    if (!aligned(p, 16) || !aligned(g, 16) || !aligned(momentum_buffer, 16)) return ISA_EALIGN;
    const SgdOp op{sqnorm, lr_dev, lr, (float)momentum, wd, max_norm, gscale};
    return launch(p, g, momentum_buffer, nullptr, n, op, stream);
}
