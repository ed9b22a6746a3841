/*
 * isa_kernels.h — C-ABI of the MI355X (gfx950) kernel library for the ReSeg hot path.
 *
 * The reference (Snoworday/instance-segmentation-attention) has no FFI: its boundary is the Python
 * class `ReSeg` (code/lib/archs/reseg.py:52-130) whose layers dispatch to torch/cuDNN.  This header
 * is the layer the drop-in `ReSeg` class calls instead; each entry point names
 * the reference operator(s) it replaces.  Conventions:
 *   - plain C, no torch types; the caller owns every buffer (activations, parameters, scratch);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never allocates,
 *     never synchronises, so a whole step can be captured into a hipGraph;
 *   - return 0 on success, a negative ISA_E* code on argument errors (nothing is launched then);
 *   - activations are NHWC "views": element (b,y,x,c) lives at data[((b*h+y)*w+x)*ld + c], so
 *     channel concatenation is done by writing into a slice of a wider buffer (reseg/unet `cat`);
 *   - an input may be LAZY: its true value is act(scale[c]*raw+shift[c])*bscale[b][c] (isa_pro).
 *     That is how train-mode BatchNorm+ReLU6 (137 BN modules) costs no extra pass over HBM: the
 *     producer writes raw conv output and per-channel sum/sumsq, isa_bn_finalize turns those into
 *     scale/shift, the consumer applies them while loading.
 */
#ifndef ISA_KERNELS_H
#define ISA_KERNELS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { ISA_F32 = 0, ISA_BF16 = 1,
       ISA_F16 = 2 };  /* fp16 storage: accepted by the attention operators (isa_sdp_attention, isa_sdp_scores) only */
enum { ISA_ACT_NONE = 0, ISA_ACT_RELU = 1, ISA_ACT_RELU6 = 2, ISA_ACT_LEAKY = 3, ISA_ACT_TANH = 4 };
enum { ISA_STAT_REPLICAS = 8 };   /* layout of every per-channel statistics buffer: [8][2*C] */
enum { ISA_OK = 0, ISA_EINVAL = -1, ISA_EALIGN = -2, ISA_EDTYPE = -3, ISA_ELAUNCH = -4, ISA_ENOMEM = -5 };

/* conv_gemm input addressing */
enum { ISA_IN_1X1 = 0,       /* K = Cin                       (nn.Conv2d k=1)                    */
       ISA_IN_3X3 = 1,       /* K = 9*Cin, zero pad 1         (nn.Conv2d k=3 p=1, dense)         */
       ISA_IN_GATHER2 = 2 }; /* K = 4*Cin, tap (dy,dx) reads pixel (2y+dy,2x+dx) of a 2x image
                                (data-gradient of ConvTranspose2d k=2 s=2)                       */
/* conv_gemm output addressing */
enum { ISA_OUT_PLAIN = 0,
       ISA_OUT_SHUFFLE2 = 1 }; /* N = 4*Cout, column (dy,dx,co) goes to pixel (2y+dy,2x+dx)
                                  (forward of ConvTranspose2d k=2 s=2)                          */

typedef struct isa_tensor {
    void*   data;   /* device pointer to element (0,0,0,0) of the view */
    int32_t n, h, w;
    int32_t c;      /* channels in the view */
    int32_t ld;     /* pixel stride in elements (>= c) */
    int32_t dtype;  /* ISA_F32 | ISA_BF16 */
    int32_t groups; /* statistic groups G (0 or 1: one group).  G > 1: the n images are G consecutive groups of n/G
                       images with separate train-mode BatchNorm statistics (the decoder iterations of attenet2.py:384-399
                       batched into one pass share weights but not batch statistics).  Every per-channel array that
                       accompanies a grouped tensor then carries a leading [G] dimension: isa_pro.scale/shift [G][c],
                       stats [G][ISA_STAT_REPLICAS][2N], isa_bn_bwd scale/shift/mean/invstd [G][c] and red/out_red
                       [G][ISA_STAT_REPLICAS][2c]; per-image arrays (bscale, oscale) are [n][c] as before and parameter
                       gradients (dw, dbias, dgamma, dbeta) are sums over all groups.  Entry points without per-channel
                       statistics or constants ignore the field. */
} isa_tensor;

/* A train-mode BatchNorm finalize that has NOT run yet, handed to the consumer of the lazy tensor (isa_pro.fin): the
 * consuming kernel derives scale/shift from the producer's statistics itself - every workgroup for its own statistic
 * group, into LDS - and ONE workgroup of the launch does what isa_bn_finalize does to memory: scale/shift/mean/invstd
 * [G][c] (read later by the backward entry points) and, when running_mean/var are given, the G ordered running-statistic
 * updates.  The arithmetic is isa_bn_finalize's (the same device function).  It removes a ~5 us launch from the dependency
 * chain of every BatchNorm (nn.BatchNorm2d forward in train mode, torch/nn/modules/batchnorm.py; the reference's
 * MobileNetDenseASPP.py:68-123 blocks have three each).  Entry points that take an isa_pro but have no in-kernel form
 * (isa_chan_mean, the weight-gradient and fused backward entry points, the eval-epilogue GEMM) run isa_bn_finalize on
 * the same stream ahead of their own kernels, so a non-NULL fin is always honoured.  They launch it after every argument
 * and workspace check: a call that returns ISA_EINVAL, ISA_EALIGN or ISA_ENOMEM has changed nothing.  c <= ISA_FIN_MAX_C
 * in-kernel, wider layers take the launch. */
#define ISA_FIN_MAX_C 1024
typedef struct isa_bn_fin {
    const float* stats;        /* [G][ISA_STAT_REPLICAS][2c] sums of the batch, complete on this stream */
    const float* gamma;        /* [c] or NULL (1) */
    const float* beta;         /* [c] or NULL (0) */
    float* running_mean;       /* [c] or NULL: no running-statistics update by this consumer */
    float* running_var;
    float* scale;              /* [G][c] outputs, as isa_bn_finalize; scale/shift must equal isa_pro.scale/shift */
    float* shift;
    float* mean;               /* may be NULL */
    float* invstd;             /* may be NULL */
    float count, momentum, eps;
    int32_t repeat;            /* as isa_bn_finalize */
} isa_bn_fin;

typedef struct isa_pro {       /* lazy-input prologue; all pointers may be NULL */
    const float* scale;        /* [c]   ([G][c] for a grouped tensor, see isa_tensor.groups) */
    const float* shift;        /* [c]   */
    const float* bscale;       /* [n,c] per-image channel multiplier (Dropout2d mask, SE gate) */
    int32_t      act;          /* ISA_ACT_* applied after the affine, before bscale */
    const isa_bn_fin* fin;     /* NULL, or the pending finalize that produces scale/shift (HOST pointer, read during the call) */
} isa_pro;

typedef struct isa_conv_ep {   /* output epilogue of isa_conv_gemm_ep: y = act(scale[n]*(conv+bias) + shift[n]) + res */
    const float* scale;        /* [N] eval-mode BatchNorm scale  gamma / sqrt(running_var + eps)          */
    const float* shift;        /* [N]                     shift  beta - running_mean * scale               */
    int32_t      act;          /* ISA_ACT_* applied after the affine                                        */
    const isa_tensor* res;     /* optional residual branch, same shape and dtype as y (may be NULL)         */
} isa_conv_ep;

typedef struct isa_slab_arena isa_slab_arena;   /* opaque: deferred weight-gradient folds, see below */

typedef struct isa_pack_entry { /* one parameter tensor to repack (see isa_pack_weights) */
    int64_t src_off;            /* element offset into the fp32 master buffer */
    int64_t dst_off;            /* element offset into the packed buffer */
    int32_t kind;               /* 0 conv fwd   src[N][K][taps]  -> dst[rows=N][taps][kp]
                                   1 conv dgrad src[N][K][taps]  -> dst[rows=Kphys][taps flipped][kp>=N]
                                   2 convT fwd  src[K][Co][2][2] -> dst[rows=4*Co][kp]      (n = Co)
                                   3 convT dgrad                 -> dst[rows=Kphys][4][kp>=Co] (n = Co)
                                   4 depthwise  src[C][1][3][3]  -> dst[9][rows]            (n = C)
                                   5 depthwise, taps flipped (data gradient)                        */
    int32_t n, k, taps;         /* logical dims of the source tensor */
    int32_t kp;                 /* padded contraction length per tap in the destination (%32==0) */
    int32_t kmap_off;           /* >=0: offset into kmap[] giving, per destination channel of the
                                   K axis (kinds 0,2: contraction index; kinds 1,3: row; kinds 4,5:
                                   column), the source channel or -1 for zero: channel padding and
                                   concat reordering.  The map has one entry per destination channel:
                                   kp entries for kinds 0 and 2, `rows` entries for the others.  <0: identity */
    int32_t rows;               /* destination rows (see kind) */
} isa_pack_entry;

/* ---- parameter repacking -------------------------------------------------------------------
 * One launch repacks every conv weight from the reference's NCHW fp32 `state_dict` layout into
 * the MFMA-operand layouts (row = output channel, contiguous contraction, zero padded to 32). */
int isa_pack_weights(const isa_pack_entry* table_dev, int32_t n_entries, const int32_t* kmap_dev,
                     const float* src_base, void* dst_base, int32_t dst_dtype, void* stream);

/* ---- convolution as MFMA GEMM ----------------------------------------------------------------
 * y[M=n*h*w, N] (+)= pro(x)[M, K] * W^T (+ bias).  Replaces nn.Conv2d k=1 / k=3 dense and
 * nn.ConvTranspose2d(k=2,s=2) forward and their data-gradients (MobileNetDenseASPP.py:68-123 1x1
 * convs, utils.py:703-707 L0Layer, unet_parts.py:73 / utils.py:975 up-convs, reseg.py:73 head).
 * w: packed weights from isa_pack_weights ([Nrows][taps][kp], dtype = x.dtype).
 * stats: optional float[ISA_STAT_R][2*N] (zeroed by the caller); per-channel sum and sum of squares of
 *        the fp32 result are atomically added into replica (workgroup & 7): train-mode BatchNorm
 *        statistics fused into the producer without serialising on a handful of L2 atomics.
 * accumulate != 0: y += result (gradient accumulation for multi-consumer tensors).            */
int isa_conv_gemm(const isa_tensor* x, const isa_pro* pro, const void* w, int32_t kp,
                  const float* bias, const isa_tensor* y, int32_t in_mode, int32_t out_mode,
                  float* stats, int32_t accumulate, void* stream);

/* The same convolution with an output epilogue: eval-mode BatchNorm2d (a constant per-channel affine), the activation and
 * the block's residual add are applied before the store, so `model.eval()` needs neither a lazy prologue in the consumer
 * nor the materialising pass of a block output (reference: nn.Sequential(conv, BatchNorm2d, ReLU6) in eval mode and
 * `x + self.conv(x)`, MobileNetDenseASPP.py:68-123).  No statistics, no accumulate, plain output layout.           */
int isa_conv_gemm_ep(const isa_tensor* x, const isa_pro* pro, const void* w, int32_t kp,
                     const float* bias, const isa_tensor* y, int32_t in_mode, const isa_conv_ep* ep, void* stream);

/* Whole-block forward of InvertedV1Residual in eval mode (MobileNetDenseASPP.py:68-93 under model.eval()) in ONE pass:
 *   y = ep( pw1x1( ReLU6( bn1_scale * dw3x3(x) + bn1_shift ) ) )        ep as in isa_conv_gemm_ep (BN2 affine, residual)
 * The depthwise output - the block's widest tensor - stays in LDS (read C + write C' instead of 3C + C' per pixel).
 * bf16 storage; x plain (no prologue), x->c % 32 == 0 and <= 128, y->c % 16 == 0 and <= 64, h % 8 == 0, w % 32 == 0
 * (the 256x256 ... 32x32 levels of the backbone; other shapes: ISA_EINVAL, callers use isa_dwconv3x3 +
 * isa_conv_gemm_ep).  w_dw: packed [9][C] (isa_pack_weights kind 4), w_pw: packed [N][kp] (kind 0). */
int isa_dwpw_eval(const isa_tensor* x, const void* w_dw, const float* bn1_scale, const float* bn1_shift,
                  const void* w_pw, int32_t kp, const isa_conv_ep* ep, const isa_tensor* y, void* stream);

/* Weight gradient of the same family, accumulated straight into the reference's state_dict layout:
 * dw[N][Ksrc][kh][kw] (or [K][Co][2][2] for ISA_OUT_SHUFFLE2)
 *   += sum_m dy[m,n] * pro(x)[m@tap, kd],  kd -> k through kmap (NULL = identity, -1 = padding).
 * dbias[N] += sum_m dy (optional; for SHUFFLE2 the sum runs over all four output quadrants).
 * Two launches, no atomics (deterministic): split-M workgroups write partial slabs into `ws`
 * (caller scratch, >= a few MB; the split factor adapts to ws_floats), a reduce kernel folds them.
 * `defer` (optional, all weight-gradient entry points): see isa_slab_arena below. */
int isa_conv_wgrad(const isa_tensor* x, const isa_pro* pro, const isa_tensor* dy,
                   float* dw, float* dbias, int32_t in_mode, int32_t out_mode,
                   const int32_t* kmap, int32_t ksrc, float* ws, int64_t ws_floats, isa_slab_arena* defer,
                   void* stream);

/* ---- depthwise 3x3, pad 1 (MobileNetDenseASPP.py:77,109; reseg.py:79,93) ---------------------
 * y = dw3x3(pro(x)) (+bias); w packed [9][C] (kind 4); stats as above.                         */
int isa_dwconv3x3(const isa_tensor* x, const isa_pro* pro, const void* w, const float* bias,
                  const isa_tensor* y, float* stats, void* stream);
/* dx (+)= dw3x3^T(dy): w = tap-flipped packing (kind 5).
 * wgrad: dw[C][1][3][3] (reference layout) += sum dy * pro(x) shifted; dbias += sum dy; only the
 * first csrc channels are real parameters (the 21-channel input is padded to 24).              */
int isa_dwconv3x3_dgrad(const isa_tensor* dy, const void* w, const isa_tensor* dx,
                        int32_t accumulate, void* stream);
int isa_dwconv3x3_wgrad(const isa_tensor* x, const isa_pro* pro, const isa_tensor* dy,
                        float* dw, float* dbias, int32_t csrc, float* ws, int64_t ws_floats, isa_slab_arena* defer,
                        void* stream);

/* Backward constants of one train-mode BatchNorm2d layer (what torch autograd keeps for
 * native_batch_norm_backward): scale/shift/mean/invstd from isa_bn_finalize, `red` = the
 * [ISA_STAT_REPLICAS][2C] sums written by isa_bn_bwd_reduce (the consumer adds the replicas),
 * `out_red` = where a fused producer writes those sums, dgamma/dbeta accumulate (may be NULL).     */
typedef struct isa_bn_bwd {
    const float* scale; const float* shift; const float* mean; const float* invstd;
    float* red; float* out_red;
    float* dgamma; float* dbeta;
    float count; int32_t act;
} isa_bn_bwd;

/* Fused backward of the  x -> dw3x3 -> y -> BN(train)+act  segment of InvertedResidual /
 * InvertedV1Residual (MobileNetDenseASPP.py:77-80,109-111), one pass over HBM:
 *   dy   = BN-backward(g, y; ybn)                 (what isa_bn_bwd_apply would store)
 *   dx  (+)= dw3x3^T(dy),  dw += pro(x) (*) dy    (isa_dwconv3x3_dgrad + isa_dwconv3x3_wgrad)
 *   xbn != NULL: xbn->out_red += sums of BN(x)'s backward over the finished dx
 *                (isa_bn_bwd_reduce of the layer that produced x; requires dx to be complete, i.e.
 *                every other consumer of x has already accumulated into it).
 * addend (optional, shape of x): dx += addend - the gradient arriving through the block's residual branch.
 * g, y, x, dx: same shape and dtype, C % 8 == 0; xpro without bscale; ybn->red already reduced.     */
int isa_dwconv3x3_bn_backward(const isa_tensor* g, const isa_tensor* y, const isa_bn_bwd* ybn,
                              const isa_tensor* x, const isa_pro* xpro, const isa_bn_bwd* xbn,
                              const void* w_flipped, float* dw, int32_t csrc,
                              const isa_tensor* dx, int32_t accumulate, const isa_tensor* addend,
                              float* ws, int64_t ws_floats, isa_slab_arena* defer, void* stream);
/* The same call for a depthwise conv WITH a bias (the instance stems, reseg.py:78-102): dbias[c] += sum of dy over all
 * pixels, folded with dw (same launch, immediate or deferred).  Nothing else depends on the bias: y is the stored conv
 * output, bias included.  dbias == NULL is isa_dwconv3x3_bn_backward, bit for bit.                   */
int isa_dwconv3x3_bias_bn_backward(const isa_tensor* g, const isa_tensor* y, const isa_bn_bwd* ybn,
                                   const isa_tensor* x, const isa_pro* xpro, const isa_bn_bwd* xbn,
                                   const void* w_flipped, float* dw, int32_t csrc,
                                   const isa_tensor* dx, int32_t accumulate, const isa_tensor* addend,
                                   float* ws, int64_t ws_floats, isa_slab_arena* defer, void* stream, float* dbias);

/* The same fusion for a bias-free 1x1 convolution y = W x (W fp32 [N][K], state_dict layout) followed by a
 * train-mode BatchNorm2d (MobileNetDenseASPP.py:105-107,113-114 expand / project; :81-82 InvertedV1):
 *   dy = BN-backward(g, y; ybn);  dw += dy^T . pro(x);  dx (+)= dy . W;  xbn as above.
 * `addend` (optional, shape of x): dx += addend, e.g. the gradient arriving through the block's residual branch
 * (saves the separate accumulate pass).
 * y == NULL: the kernel does not read the conv's output but recomputes it per pixel tile as W . pro(x), with the
 * operand rounding and the MFMA sequence of isa_conv_gemm, and rounds it to bf16 as that call stored it: one cold
 * N-channel read less, results bit-identical to the call with y.  The caller then guarantees that BN(y)'s input is
 * what isa_conv_gemm stored for this x, this prologue and this w (bf16, 1x1, no bias, ISA_OUT_PLAIN, no accumulate).
 * Only with ybn->act ISA_ACT_RELU6 or ISA_ACT_NONE; any other activation with y == NULL is ISA_EINVAL.
 * bf16 storage only, N <= 64, K <= 64, both multiples of 8; otherwise ISA_EINVAL (callers then use
 * isa_bn_bwd_apply + isa_conv_wgrad + isa_conv_gemm).                                               */
int isa_conv1x1_bn_backward(const isa_tensor* g, const isa_tensor* y, const isa_bn_bwd* ybn,
                            const isa_tensor* x, const isa_pro* xpro, const isa_bn_bwd* xbn,
                            const float* w, float* dw, const isa_tensor* dx, int32_t accumulate,
                            const isa_tensor* addend, float* ws, int64_t ws_floats, isa_slab_arena* defer,
                            void* stream);
/* The same call for a 1x1 conv WITH a bias, y = W x + bias (fp32 [N] each): dbias[n] += sum of dy[.][n] over all pixels,
 * folded with dw (same launch, immediate or deferred).  With y == NULL the recompute adds bias[n] where isa_conv_gemm's
 * epilogue does (fp32, before the bf16 rounding), so the caller's guarantee above reads "with this bias".
 * bias and dbias come together: one without the other is ISA_EINVAL, checked before anything is launched.  Both NULL
 * is isa_conv1x1_bn_backward, bit for bit.                                                          */
int isa_conv1x1_bias_bn_backward(const isa_tensor* g, const isa_tensor* y, const isa_bn_bwd* ybn,
                                 const isa_tensor* x, const isa_pro* xpro, const isa_bn_bwd* xbn,
                                 const float* w, float* dw, const isa_tensor* dx, int32_t accumulate,
                                 const isa_tensor* addend, float* ws, int64_t ws_floats, isa_slab_arena* defer,
                                 void* stream, const float* bias, float* dbias);

/* ---- deferred weight-gradient folds ------------------------------------------------------------
 * Every weight-gradient entry point is two-stage: partial slabs, then a small fold kernel that adds them into
 * dw/dbias.  Nothing reads a weight gradient before the optimizer (torch autograd gives the same freedom to the
 * reference's loss.backward(), train.py:312-322 -> model.py:204-216), so a backward pass may postpone the folds.
 * The state is an explicit handle (no global or thread-local state): an isa_slab_arena wraps a caller-owned fp32
 * region (256-byte aligned, >= 16M floats).  Weight-gradient entry points that receive the handle (`defer` != NULL)
 * ignore their `ws`, place their slabs in the arena one after the other and record the fold; isa_slab_arena_flush
 * adds every recorded slab set into its dw/dbias with one launch per 32 folds (~190 small launches fewer per
 * training step at the BASELINE configuration).  When the arena cannot hold a call's slabs the call returns
 * ISA_ENOMEM and launches nothing.  A handle is used by one host thread at a time; distinct handles are
 * independent.  The region must not be reused before the flush's kernels have run.                        */
int isa_slab_arena_create(float* region, int64_t region_floats, isa_slab_arena** out);
int isa_slab_arena_destroy(isa_slab_arena* a);
int isa_slab_arena_begin(isa_slab_arena* a);                 /* rewind; forget folds recorded but never flushed */
int isa_slab_arena_flush(isa_slab_arena* a, void* stream, int32_t* n_folds, int64_t* floats_used);

/* ---- BatchNorm2d pieces (torch.nn.BatchNorm2d train/eval semantics) --------------------------
 * finalize: stats[2C] (sum, sumsq over `count` values) -> scale/shift (and mean/invstd for the
 * backward); updates running_mean/var (momentum, unbiased var) when running_* != NULL.
 * eval mode: pass stats == NULL and scale/shift are derived from running_*.
 * groups G > 1 (isa_tensor.groups): stats [G][ISA_STAT_REPLICAS][2c] and `count` values per group ->
 * scale/shift/mean/invstd [G][c]; the running statistics take the G updates in group order, as the reference's
 * decoder iterations pass through the same module one after the other (attenet2.py:384-399).
 * repeat R > 1: every update is applied R times (a sub-network whose input does not depend on the iteration is
 * evaluated once here where the reference evaluates it R times with identical batch statistics).           */
int isa_bn_finalize(const float* stats, float count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps,
                    float* scale, float* shift, float* mean, float* invstd, int32_t c,
                    int32_t groups, int32_t repeat, void* stream);
/* Running-statistics updates of `n` train-mode layers, applied in array order by ONE launch per 64 layers: what
 * isa_bn_finalize does to running_mean/var when it is given them.  For statistics produced on another HIP stream
 * than the one that must own the update order (the decoder iterations run concurrently, attenet2.py:384-399 runs
 * them one after the other: iteration 0 updates inside its finalize, iteration 1's updates are applied here after
 * the join).  upd: HOST array, copied into the kernel arguments (a captured hipGraph keeps it by value). */
typedef struct isa_bn_upd {
    const float* stats;           /* [ISA_STAT_REPLICAS][2C] sums of the batch (device) */
    float* running_mean; float* running_var;
    float count; int32_t c;
} isa_bn_upd;
int isa_bn_running_update(const isa_bn_upd* upd, int32_t n, float momentum, void* stream);
/* backward of t = act(scale*y+shift): reduce pass  red[2C] += (sum dz, sum dz*yhat),
 * then apply pass  dy = gamma*invstd*(dz - red0/count - yhat*red1/count)  (in place over dt ok).
 * dz = dt * act'(z) (* bscale[b][c]), yhat = (y - mean) * invstd.
 * red != NULL (either mode): dbeta += red0 and dgamma += red1 (each may be NULL), once per group and channel.
 * train != 0: red is required and the apply subtracts the batch-statistics terms above.
 * train == 0 (eval-mode BatchNorm2d, constants from the running statistics): dy = scale * dz; pass the sums of a
 * reduce pass over the same dt as `red` to get torch's dbeta = sum dz, dgamma = sum dz * yhat, or NULL for none.
 * Activation only (NULL constants, NULL red, count 1, train 0): dy = dt * act'(y). */
int isa_bn_bwd_reduce(const isa_tensor* dt, const isa_tensor* y, const float* scale,
                      const float* shift, const float* mean, const float* invstd, int32_t act,
                      const float* bscale, float* red, void* stream);
int isa_bn_bwd_apply(const isa_tensor* dt, const isa_tensor* y, const float* scale,
                     const float* shift, const float* mean, const float* invstd, int32_t act,
                     const float* bscale, const float* gamma, const float* red, float count,
                     int32_t train, const isa_tensor* dy, float* dgamma, float* dbeta,
                     void* stream);

/* ---- materialise a lazy tensor: out = pro(x) (+ res)  (residual adds of Inverted*Residual,
 * F.dropout2d, torch.cat placement) and its backward pieces ----------------------------------- */
/* out = (pro(x) (+res) (+res2)) * oscale[n,c]   (oscale: F.dropout2d after a residual sum).
 * Broadcast form: out has G groups (out->groups = G, out->n = G * x->n) while x, res hold ONE group: every output
 * group g is (pro(x) + res (+ res2[g])) * oscale[g] - the Dropout2d that follows an iteration-independent block. */
int isa_affine_act_res(const isa_tensor* x, const isa_pro* pro, const isa_tensor* res,
                       const isa_tensor* res2, const float* oscale, const isa_tensor* out,
                       void* stream);
/* dst (+)= src  (NHWC views; gradient fan-in of residual/skip connections) */
int isa_axpy(const isa_tensor* src, const isa_tensor* dst, float alpha, int32_t accumulate,
             void* stream);

/* ---- pooling / resampling ------------------------------------------------------------------ */
/* 2x2 mean, stride 2 == F.interpolate(scale=0.5,bilinear) on even sizes (unet_parts.py:58) */
int isa_avgpool2(const isa_tensor* x, const isa_tensor* y, void* stream);
int isa_avgpool2_bwd(const isa_tensor* dy, const isa_tensor* dx, int32_t accumulate, void* stream);
/* 3x3 mean, stride 1, pad 1, count_include_pad (utils.py:634,645); optional per-pixel mask mul;
 * y (+)= ...: the operator is self-adjoint, so the same call with accumulate is its backward */
int isa_avgpool3(const isa_tensor* x, const isa_tensor* mask, const isa_tensor* y, int32_t accumulate,
                 void* stream);

/* ---- squeeze-excite gate + heads (utils.py:402-420, reseg.py:72-75,116-120) ------------------ */
/* mean over h*w of pro(x), ADDED to out[n,c] (float atomics from several workgroups per image): zero it first.
 * The whole prologue is honoured: per-group scale/shift [G][c] for a grouped x, then the activation, then bscale[n][c]. */
int isa_chan_mean(const isa_tensor* x, const isa_pro* pro, float* out, void* stream);
/* gate[n,c] = sigmoid(W2 relu(W1 m + b1) + b2); hidden/intermediates kept for backward */
int isa_se_fc(const float* mean, const float* w1, const float* b1, const float* w2,
              const float* b2, int32_t n, int32_t c, int32_t hidden, float* hid, float* gate,
              void* stream);
/* argmax over channels -> float map in {0..c-1} (first max wins, torch.argmax; NaN counts as the maximum, so the first
 * NaN channel wins, as in torch) */
int isa_chan_argmax(const isa_tensor* x, const isa_tensor* y, void* stream);

/* ---- attention mask head (utils.py:457-663, attenet2.py:304-347) ---------------------------------
 * Single-channel maps (masks, scores, probabilities, targets) are fp32 [n, h*w] arrays.
 * SpatialAttentionLayer (utils.py:484-523), four steps: */
int isa_mask_dot(const isa_tensor* x, const float* m, const float* w, const float* bias,
                 float* dot /*zeroed*/, float* chansum /*[n,c] zeroed*/, void* stream);
/* `part` (isa_sp_softmax, isa_ins_softmax): caller scratch of n * ISA_ROW_CHUNKS * 4 floats, or NULL.  With it (and
 * L <= 4096 * ISA_ROW_CHUNKS) a row is worked on by L / 4096 workgroups in two launches - chunk scores and online-softmax
 * partials, then the normalisation - instead of by one workgroup per row (n = 16 ... 32 rows of 65 536 pixels left most of the
 * chip idle for 86 us); same values up to the order of the fp32 sums. */
#define ISA_ROW_CHUNKS 64
int isa_sp_softmax(const float* dot, const float* m, const float* chansum, const float* lh,
                   const float* fcw, const float* fcb, int32_t n, int32_t c, int64_t L,
                   float* beta, float* rowstat /*[n,4]: max,sumexp,count,h_t*/, float* part, void* stream);
int isa_scaled_stats(const isa_tensor* x, const float* beta, float* stats /*[2c] zeroed*/, void* stream);
int isa_sp_apply(const isa_tensor* x, const float* beta, const float* m, const float* scale,
                 const float* shift, const isa_tensor* out, void* stream);
/* maskBN (utils.py:568-591) on the 1-channel score map, fused with AvgPool3x3 * sem (utils.py:645) */
int isa_maskbn_stats(const isa_tensor* e, const float* m, const float* mean_in, float* out, void* stream);
int isa_maskbn_finalize(const float* am, const float* v, int32_t n, int32_t stage, float* mean_var,
                        float* running_mean, float* running_var, float f, int32_t train, void* stream);
int isa_maskbn_apply_pool(const isa_tensor* e, const float* sem, const float* mean_var, const float* w,
                          const float* b, float eps, float* merge, void* stream);
/* HardAttentionLayer softmax for the selected instance of each image (utils.py:648-655 + the
 * gather of attenet2.py:342-343): alpha[b,:] = softmax over pixels of ins[b, idx[b]] */
int isa_ins_softmax(const float* merge, const int64_t* ins, const int32_t* idx, int32_t n, int32_t nobj,
                    int64_t L, float* alpha, float* rowstat /*[n,2]*/, int32_t nsrc, float* part, void* stream);
/* `nsrc` (here and in isa_pool_target / isa_ins_softmax_bwd; 0 = n): the n rows are n/nsrc decoder iterations over the same
 * nsrc images - row b reads merge / ins of image b % nsrc with its own idx[b], so the fronts of all iterations
 * (attenet2.py:384-399) are one launch.  isa_concat_aux's `mask_n` is the same for its shared mask_all map. */
/* DecoderLayer.sample (attenet2.py:304-324): first argmax per row, on device.  race == NULL: the eval branch
 * (argmax of alpha).  race != NULL ([n, L] draws from Exp(1)): argmax of alpha / race = one draw from
 * Multinomial(alpha), the training branch (torch.multinomial's own single-sample form).  alpha / race is an fp32
 * division, correctly rounded.  NaN never wins (unlike torch.argmax): a pixel with alpha = 0 and race = 0 cannot be
 * drawn; a row without any value above -inf (all NaN, or all -inf) gives 0.  L >= 1. */
int isa_row_argmax(const float* a, const float* race, int32_t n, int64_t L, int32_t* out, void* stream);
/* sem_seg_argmax = GT.argmax(1) (reseg.py:118) of the int64 one-hot target [n,2,h,w] as an fp32 {0,1} map [n, h*w] */
int isa_onehot_map(const int64_t* onehot, int32_t n, int64_t hw, float* out, void* stream);
/* F.dropout2d masks (utils.py:984,1104-1110) from uniform draws: out = (u < keep) / keep */
int isa_dropout_mask(const float* u, int64_t n, float keep, float* out, void* stream);
/* softmax over the channels of an NHWC logit map, written NCHW fp32 (Model.predict, model.py:486) */
int isa_softmax_nchw(const isa_tensor* x, float* out, void* stream);
/* UpDecoderLayer.resize (utils.py:841-846): f x f max-pool of the instance plane / of an fp32 map.  The instance planes
 * must hold values in {0, 1}: any nonzero value pools to 1.  The fp32 map's maximum starts from -inf (negative maps pool
 * exactly).  H % f, W % f and n % nsrc must be 0. */
int isa_pool_target(const int64_t* ins, const int32_t* idx, const float* src, int32_t nobj, int32_t n,
                    int32_t H, int32_t W, int32_t f, float* out, int32_t nsrc, void* stream);
/* mask_all + conPosition channels (utils.py:1027-1045,1085) written into a concat slice: channel 0 = mask_all of image
 * b % mask_n, channels 1 .. 2nb = the code bits of (row % f, col % f) of s_t[b] (row bits MSB first, then the column
 * bits), channel 2nb + 1 = the marker; the code and marker channels are 0 outside the coarse cell of s_t[b]. */
int isa_concat_aux(const isa_tensor* dst, const float* mask_all, const int32_t* s_t, int32_t W_full,
                   int32_t f, int32_t nb, int32_t mask_n, void* stream);
/* UpAttenLayer.Mask (utils.py:1047-1056): out = up * softmax2(bilinear_x2(pred))[1] */
int isa_gate(const isa_tensor* up, const isa_tensor* pred, const isa_tensor* out, float* gmap, void* stream);
/* per-image sums for dice / focal / CE of a 2-class prediction (dice.py:10-51, multi_loss.py:27-42):
 * sums[b][0..6] = {sum p1*t, sum p1, sum t, sum focal, sum ce, sum p1^2, count}; stride 8 floats */
int isa_mask_loss_sums(const isa_tensor* pred, const float* target, const int64_t* onehot, float* sums,
                       void* stream);

/* ---- ground-truth-free instance inference (ReSeg.segment; the reference has no working form of it) ----------------
 * State per image b over L = h*w pixels: labels uint8 [n, L] (0 = no instance), count int32 [n] (instances found),
 * remaining[b,p] = sem[b,p] > 0.5 and labels[b,p] == 0, active[b] = any(remaining[b]), the glimpse point s_t[b].
 * The point of an image is the first arg-max of merge[b,p] over remaining[b]: a NaN score counts as -inf (it never
 * beats a number), equal scores go to the smaller pixel index, and if no remaining pixel scores above -inf the point is
 * the first remaining pixel - so the point of an active image is always one of its remaining pixels; an inactive
 * image gets 0.
 * isa_seg_begin: labels = 0, count = 0, then s_t / active from the foreground map sem (fp32 [n, L]), and
 *   any_active[0] = 1 if any image is active, else 0.
 * isa_seg_claim: one pass over [n, L].  pred: the decoder's level-4 logits [n,h,w,2] (fp32 | bf16, any ld; ld == 2 with
 *   16-byte aligned data takes 16-byte loads) for the points s_t.  In an image with active[b] != 0 and count[b] < 255
 *   every remaining pixel with l1 > l0 (false for NaN), and the pixel s_t[b] if it is remaining, gets label
 *   count[b] + 1, and count[b] grows by one; other images keep labels and count.  Then s_next / active / any_active
 *   are set from what stays remaining, as isa_seg_begin sets them.  s_next may be s_t (it is written by the second
 *   launch, after every read of s_t).
 * Both run a chunk pass (a row is shared by up to ISA_ROW_CHUNKS workgroups) and a one-workgroup fold of the chunk
 * candidates, which alone writes count / active / s_next / any_active; the result does not depend on the order in which
 * workgroups run.  part: caller scratch of n * ISA_ROW_CHUNKS * 2 floats.  L % 4 == 0; sem and merge 16-byte aligned,
 * labels 4-byte aligned (ISA_EALIGN otherwise); n <= 65535. */
int isa_seg_begin(const float* sem, const float* merge, int32_t n, int64_t L, uint8_t* labels, int32_t* count,
                  int32_t* s_t, int32_t* active, int32_t* any_active, float* part, void* stream);
int isa_seg_claim(const isa_tensor* pred, const float* sem, const float* merge, const int32_t* s_t, uint8_t* labels,
                  int32_t* count, int32_t* active, int32_t* s_next, int32_t* any_active, float* part, void* stream);

/* ---- scoring instance predictions on the device (code/evaluate.py:18-56: calc_dic, calc_dice, calc_bd, calc_sbd) ------
 * Every entry checks all its arguments before it launches anything (ISA_EINVAL / ISA_EALIGN); n <= 65535.
 * isa_labels_from_planes: ground-truth instance planes -> uint8 label map [n, hw].  The label of a pixel is 1 + the
 *   smallest plane index whose value is non-zero, 0 if there is none; where planes overlap the FIRST plane gets the pixel.
 *   form ISA_PLANES_U8_NHWK: uint8 [n,h,w,k] (the compact targets); ISA_PLANES_I64_NKHW: int64 [n,k,h,w] (the
 *   reference's, 8-byte aligned); ISA_PLANES_F32_NKHW: fp32 [n,k,h,w] (k = 1: the sem_argmax map the model returns; NaN
 *   counts as non-zero).  1 <= k <= 255.
 * isa_label_pair_hist: hist[i][p][q] (int32 [n][na][nb]) = number of pixels of image i with a == p and b == q, for the
 *   uint8 maps a, b [n, L].  A pixel with a >= na or b >= nb is counted in oob[i] (int32 [n]) instead.  The entry zeroes
 *   hist and oob on the stream itself: nothing has to be cleared by the caller.  1 <= na, nb <= 256, na * nb <= 16384 (the
 *   64 KiB of LDS counters of a workgroup); L % 4 == 0; a, b, hist, oob 4-byte aligned (16-byte aligned maps with
 *   L % 16 == 0 are read 16 pixels per load).  A row is shared by up to ISA_ROW_CHUNKS workgroups that add their non-zero
 *   counters with integer atomics: the result does not depend on the order in which they run.  mode ISA_HIST_AGGREGATE
 *   counts a wave's dominant pair once per wave and merges a lane's equal consecutive pairs; ISA_HIST_NAIVE is one LDS
 *   atomic per pixel, kept as the figure to measure the former against (scripts/bench_score.py).  Same result.
 * isa_instance_scores: out[i][0..7] (double, 8-byte aligned) from hist[i].  An object of a map is a non-zero label with a
 *   non-empty row (map a) or column (map b) of hist, as np.unique in evaluate.py sees it; dice[p][q] = 2 hist[p][q] /
 *   (size_a[p] + size_b[q]), the sizes counting the pixels shared with the other map's label 0 too.
 *     0: best Dice a -> b, the mean over a's objects of the max over b's objects     1: best Dice b -> a
 *     2: SBD = fmin(0, 1)          3, 4: objects present in a, in b          5: |n_a[i] - n_b[i]|
 *     6: foreground Dice 2 |a != 0 & b != 0| / (|a != 0| + |b != 0|) (calc_dice when na == nb == 2)          7: 0
 *   n_a / n_b (int32 [n]): the reported object counts; NULL: the number of objects present.
 *   Empty maps: 0 is NaN when a has no object and 0.0 when a has objects and b has none, 1 mirrors it; so SBD is NaN only
 *   when both maps are empty (calc_sbd: min(nan, nan)) and 0.0 when exactly one is.  THAT case differs from the
 *   reference: its calc_bd raises ValueError (np.max of an empty list), which a kernel cannot.  6 is NaN for two empty
 *   maps, where calc_dice divides by zero. */
enum { ISA_PLANES_U8_NHWK = 0, ISA_PLANES_I64_NKHW = 1, ISA_PLANES_F32_NKHW = 2 };
enum { ISA_HIST_AGGREGATE = 0, ISA_HIST_NAIVE = 1 };
int isa_labels_from_planes(const void* planes, int32_t form, int32_t n, int32_t k, int64_t hw, uint8_t* labels,
                           void* stream);
int isa_label_pair_hist(const uint8_t* a, const uint8_t* b, int32_t n, int64_t L, int32_t na, int32_t nb, int32_t* hist,
                        int32_t* oob, int32_t mode, void* stream);
int isa_instance_scores(const int32_t* hist, int32_t n, int32_t na, int32_t nb, const int32_t* n_a, const int32_t* n_b,
                        double* out, void* stream);

/* ---- losses and hand-derived backward of the head (the reference relies on autograd) ------------
 * isa_head_loss: attenet2.py:239-290 on device (no host sync): per-level gradient coefficients,
 * REINFORCE advantage with the EMA baseline (device scalar), and scal[0..3] += {ins_cost without the
 * NaN entropy term (attenet2.py:77, zero gradient), criterion, ins_ce_loss, ins_dice_loss}/max_iter.
 * iters > 1: the rows of `iters` decoder iterations at once - sums [5][iters*B][8], alpha / s_t / adv [iters*B], coef
 * [5][iters*B][4] - processed in iteration order, the EMA baseline carried from one to the next (attenet2.py:266). */
int isa_head_loss(const float* sums /*[5][B][8]*/, const float* alpha, const int32_t* s_t, int64_t L, int32_t B,
                  const float* level_w /*host[5]*/, float ce_weight, float lambda_l, float lambda_r, float inv_iter,
                  float* baseline, int32_t training, float* coef /*[5][B][4]*/, float* adv /*[B]*/,
                  float* scal /*[4]*/, int32_t iters, void* stream);
/* trainer-side CE + Dice on the semantic logits (model.py:255-269): scal = {ce, dice}, coef[B][4] */
int isa_sem_loss(const float* sums /*[B][8]*/, int32_t B, float* coef, float* scal, void* stream);
int isa_mask_loss_grad(const isa_tensor* pred, const float* target, const int64_t* onehot, const float* coef /*[B][4]*/,
                       const isa_tensor* dpred, int32_t accumulate, void* stream);
/* ---- K-class semantic criterion (Model.__define_criterion + the CE / Dice branches of __minibatch, model.py:102-133,
 * 255-269; dice.py:10-85; torch.nn.CrossEntropyLoss(weight)), 2 <= K <= ISA_SEM_MAX_CLASSES.  Serves every
 * (criterion, class_weights, optimize_bg, n_classes) but the shipped 2-class fg-only unweighted Multi, which keeps
 * isa_mask_loss_sums + isa_sem_loss + isa_mask_loss_grad.  logits NHWC [B,H,W,K] (bf16 | fp32, ld a multiple of 8),
 * labels uint8 [B,H,W] with values < K (a precondition, not checked: the reference raises IndexError there).
 * cfg (device, read at run time so that a captured hipGraph follows in-place changes) [4 + K] floats:
 *   {use_ce, use_dice, optimize_bg, only_present (read by isa_lovasz_assemble alone), w_0 .. w_{K-1}}; no class
 *   weights = all ones.
 * isa_sem_loss_k_sums: sums [B*3K + 2], zeroed by the caller: per image {sum p*g [K], sum p [K], sum g [K]}, then the
 *   batch's {sum w_y * nll, sum w_y}.
 * isa_sem_loss_k_assemble: one workgroup; coef [3*B*K + 1] for the gradient, scal[2] = {CE, Dice} (0 for a term the
 *   criterion does not compute).
 * isa_sem_loss_k_grad: d logits (written, or added to when accumulate != 0); channels >= K of a row untouched. */
#define ISA_SEM_MAX_CLASSES 32
int isa_sem_loss_k_sums(const isa_tensor* logits, const uint8_t* labels, const float* cfg, float* sums, void* stream);
int isa_sem_loss_k_assemble(const float* sums, const float* cfg, int32_t B, int32_t K, float* coef, float* scal,
                            void* stream);
int isa_sem_loss_k_grad(const isa_tensor* logits, const uint8_t* labels, const float* cfg, const float* coef,
                        const isa_tensor* dlogits, int32_t accumulate, void* stream);
/* The same two entries with a weight per pixel, pixw fp32 [B,H,W] (4-byte aligned, m_i > 0 expected): the batch sums
 * become {sum m w_y nll, sum m w_y}, so CE = sum m_i w_{y_i} nll_i / sum m_i w_{y_i} after isa_sem_loss_k_assemble (which
 * is unchanged), and the CE term of pixel i's gradient is scaled by m_i.  The Dice sums and terms do not see pixw.  The two
 * gradient entries run one kernel body (the unweighted one reads a 1.0 in place of pixw): with pixw = 1 and the same coef
 * isa_sem_loss_k_grad_pw writes isa_sem_loss_k_grad's bits. */
int isa_sem_loss_k_sums_pw(const isa_tensor* logits, const uint8_t* labels, const float* cfg, const float* pixw,
                           float* sums, void* stream);
int isa_sem_loss_k_grad_pw(const isa_tensor* logits, const uint8_t* labels, const float* cfg, const float* coef,
                           const float* pixw, const isa_tensor* dlogits, int32_t accumulate, void* stream);
/* ---- stable segmented key-value radix sort ---------------------------------------------------------------------------
 * isa_segsort_kv_u32 sorts nseg independent segments of seglen keys each (segment s = elements [s*seglen, (s+1)*seglen)):
 * uint32 keys ascending, compared on their bits [begin_bit, end_bit) only, every key carrying one uint32 value.  The sort
 * is stable: keys equal on those bits keep their input order.  Input, output and temporaries are six buffers of
 * nseg*seglen uint32 (4-byte aligned, ISA_EALIGN otherwise); the input is left as it is.  table: uint32 scratch of at
 * least ISA_SEGSORT_TABLE_ELEMS(nseg, seglen) elements (ISA_ENOMEM when table_elems is smaller).  The seven buffers
 * must not overlap; any two with the same address are refused.  LSD radix with 8-bit
 * digits; a pass is tile histograms, an exclusive scan of [segment][digit][tile] (three launches: sums of 2048-entry
 * chunks, their scan, the chunks; the sums live behind the digit table) and a stable scatter of tiles of ISA_SEGSORT_TILE
 * keys.  Launch boundaries are the only synchronisation between workgroups, so the launch count
 * 5 * ceil((end_bit - begin_bit) / 8) is fixed by the arguments and a captured hipGraph replays it.  Integer
 * counters only: the output is bit-identical from run to run.  ISA_EINVAL, before anything is launched: a NULL or
 * repeated buffer, nseg < 1, seglen < 1, nseg*seglen >= 2^31, or not 0 <= begin_bit < end_bit <= 32. */
#define ISA_SEGSORT_TILE 2048
#define ISA_SEGSORT_TILES(seglen) (((int64_t)(seglen) + ISA_SEGSORT_TILE - 1) / ISA_SEGSORT_TILE)
#define ISA_SEGSORT_TABLE_ELEMS(nseg, seglen) \
    ((int64_t)(nseg) * (256 * ISA_SEGSORT_TILES(seglen) + (ISA_SEGSORT_TILES(seglen) + 7) / 8))
int isa_segsort_kv_u32(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                       int32_t nseg, int64_t seglen, int32_t begin_bit, int32_t end_bit, uint32_t* tmp_keys,
                       uint32_t* tmp_vals, uint32_t* table, int64_t table_elems, void* stream);
/* ---- Lovasz-Softmax semantic criterion (lovasz_softmax, losses/lovasz_losses.py:156-196) on the segmented sort ----------
 * logits and labels as for isa_sem_loss_k_* (NHWC [B,H,W,K], bf16 | fp32, ld a multiple of 8, 16-byte aligned, groups 1,
 * B <= 65535, B*H*W*K < 2^31; labels uint8 [B,H,W] with values < K); finite logits are a precondition (NaN gives an
 * unspecified value, never an access out of range).  A segment is (class, whole batch), or (class, image) when
 * per_image != 0; either way a range of one array laid out [K][B][H*W]: nimg = per_image ? B : 1 segments per class of
 * seglen = H*W*B / nimg elements, segment index c*nimg + s.  cfg is the criterion's device buffer: optimize_bg = cfg[2]
 * and only_present = cfg[3] are read at run time, so a captured hipGraph follows in-place changes; per_image fixes the
 * launch geometry.  Every entry checks all arguments before it launches (ISA_EINVAL / ISA_EDTYPE / ISA_EALIGN).
 * isa_lovasz_keys: classes [c0, c0+nc) -> keys / vals [nc][B][H*W]: key = 0x3F800000 - bits(e), e = |[label == c] - p_c|
 *   clamped to [0,1] with p the fp32 softmax (ascending key = descending error, 30 key bits); value = pixel index inside
 *   the segment, bit 31 set for a foreground pixel.  G [nc*nimg] int32, zeroed by the caller, receives the foreground
 *   count of every segment (integer atomics).
 * isa_lovasz_coef: keys / vals sorted by isa_segsort_kv_u32(.., 0, 30, ..).  Three launches: foreground counts of the
 *   tiles (tile_counts, uint32 [nseg * ceil(seglen / ISA_SEGSORT_TILE)]), their exclusive scan per segment, then for the
 *   element at rank r with cf / cb foreground / background elements before it, I = G - cf, U = G + cb:
 *   g = 1/U (foreground) | I / (U (U+1)) (background) | G == 0: [r == 0], from the integer counts in double.
 *   partial [nseg][tiles] (double) = the tile's sum of e*g, folded in a fixed order; gpix (float [nseg][seglen], may be
 *   NULL: forward only) = sign*g in pixel order, sign -1 for a foreground pixel and +1 otherwise.
 * isa_lovasz_assemble: one workgroup.  Counted classes: optimize_bg ? 0..K-1 : 1..K-1; only_present keeps those with
 *   G > 0 in the segment.  scal[0] = mean over the kept classes (0 when none is kept), then over the images when
 *   per_image; scale [K*nimg] = 1 / (kept * nimg) for a kept (class, segment), else 0; segloss [K*nimg] double scratch.
 *   partial, G: those of all K classes, [K*nimg][tiles] and [K*nimg].
 * isa_lovasz_grad: d_c = scale * gpix, d logits_k = p_k (d_k - sum_j p_j d_j), written to dlogits (the logits' dtype and
 *   shape) or added when accumulate != 0; channels >= K of a row untouched. */
int isa_lovasz_keys(const isa_tensor* logits, const uint8_t* labels, int32_t c0, int32_t nc, int32_t per_image,
                    uint32_t* keys, uint32_t* vals, int32_t* G, void* stream);
int isa_lovasz_coef(const uint32_t* keys_sorted, const uint32_t* vals_sorted, const int32_t* G, int32_t nseg,
                    int64_t seglen, uint32_t* tile_counts, double* partial, float* gpix, void* stream);
int isa_lovasz_assemble(const double* partial, const int32_t* G, const float* cfg, int32_t B, int32_t K, int32_t per_image,
                        int64_t hw, double* segloss, float* scale, float* scal, void* stream);
int isa_lovasz_grad(const isa_tensor* logits, const float* gpix, const float* scale, int32_t per_image,
                    const isa_tensor* dlogits, int32_t accumulate, void* stream);
/* ---- discriminative embedding loss (losses/discriminative.py: calculate_means 7-62, calculate_variance_term 65-95 (its
 * hinge branch), calculate_distance_term 98-132, calculate_regularization_term 135-147, calculate_q_regularization_term
 * 149-160, discriminative_loss 162-188) and its hand-derived backward ----------------------------------------------------
 * emb x: NHWC [B,H,W,C] (bf16 | fp32, 1 <= C <= 32, ld >= C and a multiple of 8, 16-byte aligned, groups 1, B <= 65535,
 * L = H*W < 2^31).  labels: uint8 [B, L] as isa_labels_from_planes makes them of k planes (1 <= k <= ISA_DISC_MAX_K; the
 * first plane wins, so the instances are disjoint): 0 background, i + 1 = instance i; a label above k counts as
 * background.  n_objects int32 [B], clamped to [0, 32]: planes at index >= n_objects[b] are ignored for the means and the
 * var / dist / reg terms but stay foreground for qreg, as in the reference.  Instance i of image b is PRESENT when
 * i < n_objects[b] and N_i > 0 (N_i its pixel count); np_b = present instances, F_b = sum of their N_i.
 *   m_i = sum_{p in i} x_p / N_i;  mu_i = unit_means ? m_i / |m_i|_2 : m_i                       (both 0 when not present)
 *   var  = 1/B sum_b 1/F_b sum_{i present} sum_{p in i} max(|x_p - mu_i| - delta_v, 0)^2   (the divisor is the image's
 *          counted foreground, not the cluster's size: the reference, not the paper)
 *   dist = 1/B sum_{b: np_b >= 2} sum_{i != j present} max(2 delta_d - |mu_i - mu_j|, 0)^2 / (np_b (np_b - 1))
 *   reg  = 1/B sum_{b: np_b >= 1} 1/np_b sum_{i present} |mu_i|
 *   qreg = sum_{b,p} ([label_p != 0] |x_p|_2 - 1)^2 / num, num = foreground pixels of the batch: a background pixel adds the
 *          constant 1 (kept from the reference); always the L2 norm
 *   loss = weight (alpha var + beta dist + gamma reg + gamma_q qreg)
 * |.| is the L1 (norm == 1) or L2 (norm == 2) norm; delta_v, delta_d >= 0.  Where the reference divides 0 by 0 these rules
 * hold instead: a counted instance with N_i = 0 adds nothing and is not counted in np_b; F_b = 0, np_b < 2 (dist),
 * np_b = 0 (reg), num = 0 (qreg) give 0; d/|d|_2 is 0 at d = 0; the L1 derivative is sign with sign(0) = 0; m_i = 0 with
 * unit_means gives mu_i = 0 and no gradient through it.
 * cfg (device, ISA_DISC_CFG_FLOATS floats, read at run time so that a captured hipGraph follows in-place changes):
 *   {delta_v, delta_d, norm (informative: the kernels take the call argument), unit_means, alpha, beta, gamma, gamma_q,
 *    weight, 0, 0, 0}.
 * Every entry checks all its arguments before it launches or writes anything (ISA_EINVAL / ISA_EALIGN / ISA_EDTYPE),
 * allocates nothing, never syncs and works on `stream`.  A row is shared by ISA_DISC_CHUNKS(L) <= ISA_ROW_CHUNKS workgroups
 * that each write a slab of their own; every fold has a fixed order and there are no float atomics: loss, means and
 * gradient are bit-reproducible.  Scratch is the caller's; none of it has to be cleared.
 * isa_disc_sums: slab (float, ISA_DISC_SLAB_FLOATS(B, L)) [B][chunks][32][32] = per chunk sum_{p in i} x_p[j], as
 *   one-hot[32 x P] . x[P x 32] on the f32-input MFMA (exact f32, a fixed fmaf chain; channels C..31 are zero operands);
 *   cslab (int32, ISA_DISC_CSLAB_INTS(B, L)) [B][chunks][32] = per chunk N_i.
 * isa_disc_means: one workgroup per image folds the chunks in order.  mu, m (may be NULL) float [B][32][32]; mnorm float
 *   [B][32] = |m_i|_2; cnt int32 [B][ISA_DISC_CNT_STRIDE] = {N_0 .. N_31 (every plane), F_b, np_b, foreground pixels, 0}.
 * isa_disc_hinge: hslab (as slab) = per chunk sum_{p in i} h_p d|d|/dd (x_p - mu_i), h_p the hinge of var; partial (double,
 *   ISA_DISC_PARTIAL_DOUBLES(B, L)) [B][chunks][2] = {sum h_p^2, sum of the qreg summand}.
 * isa_disc_assemble: two launches.  Per image: the folds, dist and reg over the <= 32 means and their gradients, d loss / d mu
 *   back through the normalisation (g_m = (g_mu - mu (mu . g_mu)) / |m|_2 when unit_means), gconst float [B][32][32] =
 *   weight g_m / N_i; coef float [B + 1]: coef[b] = weight 2 alpha / (B F_b), coef[B] = weight 2 gamma_q / num; img double
 *   [B][8] scratch.  Then one workgroup folds the images in order: scal[8] = {loss, var, dist, reg, qreg, sum_b np_b,
 *   sum_b F_b, 0} (the loss carries the weight, the four terms do not).
 * isa_disc_grad: dx_p = coef[b] h_p d|d|/dd + gconst[label_p] + coef[B] (|x_p|_2 - 1) x_p / |x_p|_2 (the last two on
 *   foreground pixels), recomputed from x, mu and the labels; written to demb (the dtype and shape of emb) or added when
 *   accumulate != 0; channels >= C of a row untouched. */
#define ISA_DISC_MAX_K 32
#define ISA_DISC_CFG_FLOATS 12
#define ISA_DISC_CNT_STRIDE 36
#define ISA_DISC_CHUNKS(L) \
    ((((int64_t)(L) + 1023) / 1024) < ISA_ROW_CHUNKS ? (((int64_t)(L) + 1023) / 1024) : (int64_t)ISA_ROW_CHUNKS)
#define ISA_DISC_SLAB_FLOATS(n, L) ((int64_t)(n) * ISA_DISC_CHUNKS(L) * 1024)
#define ISA_DISC_CSLAB_INTS(n, L) ((int64_t)(n) * ISA_DISC_CHUNKS(L) * 32)
#define ISA_DISC_PARTIAL_DOUBLES(n, L) ((int64_t)(n) * ISA_DISC_CHUNKS(L) * 2)
int isa_disc_sums(const isa_tensor* emb, const uint8_t* labels, int32_t k, float* slab, int32_t* cslab, void* stream);
int isa_disc_means(const float* slab, const int32_t* cslab, const int32_t* n_objects, const float* cfg, int32_t n, int64_t L,
                   float* mu, float* m, float* mnorm, int32_t* cnt, void* stream);
int isa_disc_hinge(const isa_tensor* emb, const uint8_t* labels, int32_t k, const int32_t* n_objects, const float* mu,
                   const float* cfg, int32_t norm, float* hslab, double* partial, void* stream);
int isa_disc_assemble(const float* hslab, const double* partial, const float* mu, const float* mnorm, const int32_t* cnt,
                      const int32_t* n_objects, const float* cfg, int32_t norm, int32_t n, int64_t L, float* gconst,
                      float* coef, double* img, float* scal, void* stream);
int isa_disc_grad(const isa_tensor* emb, const uint8_t* labels, int32_t k, const int32_t* n_objects, const float* mu,
                  const float* gconst, const float* coef, const float* cfg, int32_t norm, const isa_tensor* demb,
                  int32_t accumulate, void* stream);
/* ---- clustering the instance embedding into instances (the reference's Prediction.cluster, prediction.py:52-85, runs sklearn
 * KMeans on the host and fills the map pixel by pixel; here both methods run on the device, per image) -------------------
 * emb x: as for isa_disc_* (NHWC bf16 | fp32, 1 <= C <= 32, ld >= C and a multiple of 8, 16-byte aligned, groups 1,
 * B <= 65535, L = H*W < 2^31); channels C..ld-1 of a row are never read as data.  fg: uint8 [B, L], non-zero = foreground.
 * d(p, c) = sum_j (x_p[j] - c[j])^2, always in this direct form: the difference first, then one fp32 fmaf chain over the
 * channels in order; never |x|^2 - 2 x.c + |c|^2.  NaN embeddings are not supported (every comparison with a NaN distance
 * is false: such a pixel joins no ball and goes to centre 0).
 * Outputs of both entries: labels uint8 [B, L] (0 = background, 1..n = instances), n_objects int32 [B], centres float
 * [B][32][32] (row i = centre of label i + 1, zero past n_objects[b] and past C), sizes int32 [B][32], moved int32 [B].
 * isa_cluster_meanshift: the greedy flat-kernel mean-shift.  free = foreground pixels without label that are not noise;
 *   while k < max_objects and free is not empty and fewer than max_rounds rounds have run: s = the smallest index in free,
 *   c = x_s; `shifts` times c = mean of
 *   {p in free: d(p, c) <= bandwidth^2} (an empty set keeps c); S = that set for the last c, united with {s}; |S| >=
 *   min_pixels: k += 1, S takes label k, centre[k] = c, sizes[k] = |S|; else S is noise.  With assign_rest != 0 and k > 0
 *   every foreground pixel still without label (noise, or left when max_objects was reached) takes the label of its nearest
 *   centre (ties: the lowest label; sizes stay |S|); else it keeps 0.  n_objects[b] = k, moved[b] = 0.
 *   bandwidth > 0, 0 <= shifts <= ISA_CLUSTER_MAX_SHIFTS, 1 <= max_objects <= 32, max_objects <= max_rounds <=
 *   ISA_CLUSTER_MAX_ROUNDS, min_pixels >= 1.  The round budget is what keeps the launch count free of the data: a round
 *   ends with an object or with a ball refused as noise, and BOTH use up one of the max_rounds rounds.  With min_pixels == 1
 *   no ball is refused, rounds == k, and max_rounds == max_objects never binds; with min_pixels > 1 every refused ball
 *   before the last object needs a round of its own, and what the budget leaves unvisited is treated like what max_objects
 *   leaves (assign_rest, or 0).  1 + max_rounds (shifts + 1) + 1 launches whatever the data holds.
 * isa_cluster_kmeans: K_b = min(n_objects_in[b], foreground pixels, kmax), 1 <= kmax <= 32.  init == NULL: deterministic
 *   maximin - centre 0 is the foreground pixel of smallest index, centre j the foreground pixel farthest from its nearest
 *   chosen centre (ties: the smallest index) - in kmax launches; else init float [B][32][32] holds the first centres (rows
 *   past K_b and channels past C are ignored).  Then `iters` (0..ISA_CLUSTER_MAX_ITERS) Lloyd iterations over the foreground:
 *   every pixel goes to its nearest centre (ties: the lowest index), every centre becomes the mean of its pixels, an empty
 *   cluster keeps its centre; a last assignment makes the labels.  centres = the centres of that assignment, sizes = its
 *   counts, moved[b] = pixels whose label differs from the assignment before (0 when iters == 0), n_objects[b] = K_b.
 *   1 + (init ? 0 : kmax) + iters + 2 launches.
 * scratch: ISA_CLUSTER_SCRATCH_BYTES(B, L) bytes, 16-byte aligned, never has to be cleared: per-chunk slabs (ISA_DISC_CHUNKS
 * workgroups share an image), the per-image loop state and the moving centres, all double-buffered by launch parity.  Every
 * workgroup folds the slabs of the pass before in chunk order itself; there are no float atomics, no waits between
 * workgroups and nothing is read back, so a call is bit-reproducible and can be captured into a hipGraph on one stream.
 * Both entries check every argument before they launch or write anything (ISA_EINVAL / ISA_EALIGN / ISA_EDTYPE). */
#define ISA_CLUSTER_MAX_SHIFTS 8
#define ISA_CLUSTER_MAX_ITERS 64
#define ISA_CLUSTER_MAX_ROUNDS 256
#define ISA_CLUSTER_STATE_INTS 16
#define ISA_CLUSTER_CSLAB_STRIDE 36
#define ISA_CLUSTER_SCRATCH_BYTES(n, L) ((int64_t)(n) * (8320 + ISA_DISC_CHUNKS(L) * 8488))
int isa_cluster_meanshift(const isa_tensor* emb, const uint8_t* fg, float bandwidth, int32_t shifts, int32_t max_objects,
                          int32_t max_rounds, int32_t min_pixels, int32_t assign_rest, uint8_t* labels, int32_t* n_objects,
                          float* centres, int32_t* sizes, int32_t* moved, void* scratch, void* stream);
int isa_cluster_kmeans(const isa_tensor* emb, const uint8_t* fg, const int32_t* n_objects_in, const float* init, int32_t kmax,
                       int32_t iters, uint8_t* labels, int32_t* n_objects, float* centres, int32_t* sizes, int32_t* moved,
                       void* scratch, void* stream);
/* reference-format targets: int64 one-hot [n,k,h,w] -> uint8 labels [n,h,w] and / or the fp32 argmax(1) map [n, h*w]
 * (sem_seg_argmax, reseg.py:118); the first maximum wins, as in torch.argmax.  Either output may be NULL, not both. */
int isa_labels_from_onehot(const int64_t* onehot, int32_t n, int32_t k, int64_t hw, uint8_t* labels, float* argmax_map,
                           void* stream);
/* ---- scoring K-class semantic predictions on the device: confusion matrix, IoU, Dice, pixel accuracy ------------------
 * Both entries check every argument before they launch or clear anything (ISA_EINVAL / ISA_EALIGN / ISA_EDTYPE), are
 * asynchronous on `stream` and allocate nothing.  2 <= K <= ISA_SEM_MAX_CLASSES, n <= 65535.
 * isa_sem_confusion: one pass over the logits NHWC [n,h,w,c] (c == K, ld a multiple of 8, bf16 | fp32, 16-byte aligned:
 *   the layout of isa_sem_loss_k_sums); h*w % 4 == 0.  The prediction of a pixel is the arg-max over channels 0..K-1: the
 *   first maximum wins, NaN counts as the maximum (so the first NaN channel wins; the rule of isa_chan_argmax and
 *   torch.argmax), all -inf gives class 0.  Channels K..ld-1 are padding and never take part, whatever they hold.
 *   class_map (uint8 [n, h*w], 4-byte aligned, or NULL) receives the prediction of every pixel.
 *   labels (uint8 [n, h*w], 4-byte aligned, or NULL; not both NULL): conf[i][t][p] (int64 [n][K][K], 8-byte aligned)
 *   counts the pixels of image i with label t and prediction p; a pixel with label >= K is counted in oob[i] (int32 [n])
 *   instead.  The entry zeroes conf and oob on the stream itself.  With labels == NULL conf and oob are not touched and
 *   may be NULL.  A row is shared by up to ISA_ROW_CHUNKS workgroups that add their non-zero counters with integer
 *   atomics: the result does not depend on the order in which they run.
 * isa_sem_scores: out[i][0 .. 3+2K] (double, 8-byte aligned) from conf[i], one workgroup per image (n = 1 on a summed
 *   matrix scores a dataset total).  Per class c: tp = conf[c][c], gt = sum of row c, pr = sum of column c.
 *     0: pixel accuracy trace / total (NaN when total == 0)
 *     1: mean IoU over the classes with gt + pr - tp > 0, summed in class order (NaN when there is none)
 *     2: mean Dice over the same classes          3: the number of those classes
 *     4 .. 4+K-1: IoU[c] = tp / (gt + pr - tp), NaN for a class absent from both maps
 *     4+K .. 4+2K-1: Dice[c] = 2 tp / (gt + pr), same NaN rule
 *   Every per-class value is one correctly rounded double division of exact integers (sums below 2^53). */
int isa_sem_confusion(const isa_tensor* logits, const uint8_t* labels, int32_t K, int64_t* conf, int32_t* oob,
                      uint8_t* class_map, void* stream);
int isa_sem_scores(const int64_t* conf, int32_t n, int32_t K, double* out, void* stream);
/* ---- connected components of uint8 label maps, and the clean-up of instance maps built on them --------------------------
 * Both entries check every argument before they launch or clear anything (ISA_EINVAL / ISA_EALIGN / ISA_ENOMEM), are
 * asynchronous on `stream`, allocate nothing and never read anything back: the launch count depends on the shape and the
 * mode alone, so a captured hipGraph replays them.  n <= 65535, w % 4 == 0, h * w < 2^30.  Only integer atomics and scans
 * decide anything: two runs are bit-identical, whatever order workgroups ran in.
 * isa_cc_label: map uint8 [n,h,w] (4-byte aligned), 0 = background.  Two pixels of one image are neighbours when they share
 *   an edge (connectivity 4) or an edge or a corner (8) AND hold the same non-zero value; the last column of a row and the
 *   first of the next are not neighbours, nor are pixels of two images.  comp int32 [n,h,w] (16-byte aligned): 0 for
 *   background, else 1 + the smallest row-major pixel index (inside its image) of the pixel's component - the canonical
 *   form.  n_comp int32 [n]: components per image.  scratch: ISA_CC_LABEL_SCRATCH_BYTES(n,h,w) bytes, 16-byte aligned
 *   (the union-find parents; they need not be cleared).  Three launches (two when the image is one ISA_CC_TILE_H x
 *   ISA_CC_TILE_W tile): tiles labelled in LDS, unions across tile edges with device-scope atomics on every access,
 *   flatten.
 * isa_cc_select: map and the comp isa_cc_label made of it -> out uint8 [n,h,w] (4-byte aligned; it must not overlap map:
 *   ISA_EINVAL), count int32 [n] (labels given), dropped int32 [n].  The area of a component is its pixel count; it
 *   qualifies when area >= min_area (min_area <= 1: every component).  1 <= max_objects <= 255.
 *   ISA_CC_SPLIT: the qualifying components are numbered 1, 2, .. in ascending order of their root pixel (raster order of
 *     their first pixels); only the first max_objects get a label, the pixels of every other component become 0.
 *   ISA_CC_LARGEST: per input value v the component of largest area wins (equal areas: the smaller root); it survives when
 *     it qualifies, every other component of v becomes 0.  The survivors are numbered 1, 2, .. in ascending order of v and
 *     only the first max_objects of them get a label.
 *   In both modes dropped = qualifying components - count: components cut by the cap, and in LARGEST the qualifying
 *   fragments that lost to a larger one ("this instance was really two objects").
 *   scratch: ISA_CC_SELECT_SCRATCH_BYTES(n,h,w) bytes, 16-byte aligned, cleared by the entry (areas by root pixel, then
 *   ISA_CC_TAB_BYTES of winner keys, survivor tables and chunk counts per image).  Six launches (SPLIT: clear, areas,
 *   chunk counts of qualifying roots, one-workgroup fold, ranks, write) or five (LARGEST: clear, areas, winners, fold,
 *   write). */
#define ISA_CC_TILE_H 32
#define ISA_CC_TILE_W 64
#define ISA_CC_TAB_BYTES 4608
#define ISA_CC_LABEL_SCRATCH_BYTES(n, h, w) ((int64_t)(n) * (h) * (w) * 4)
#define ISA_CC_SELECT_SCRATCH_BYTES(n, h, w) ((int64_t)(n) * ((int64_t)(h) * (w) * 4 + ISA_CC_TAB_BYTES))
enum { ISA_CC_SPLIT = 0, ISA_CC_LARGEST = 1 };
int isa_cc_label(const uint8_t* map, int32_t n, int32_t h, int32_t w, int32_t connectivity, int32_t* comp, int32_t* n_comp,
                 void* scratch, int64_t scratch_bytes, void* stream);
int isa_cc_select(const uint8_t* map, const int32_t* comp, int32_t n, int32_t h, int32_t w, int32_t mode, int32_t min_area,
                  int32_t max_objects, uint8_t* out, int32_t* count, int32_t* dropped, void* scratch, int64_t scratch_bytes,
                  void* stream);
/* ---- measuring instances: area, box, moments, perimeter, colour; filtering and ordering by them -----------------------
 * Every entry checks all its arguments before it launches or writes anything (ISA_EINVAL / ISA_EALIGN), is asynchronous on
 * `stream`, allocates nothing, needs no scratch and never reads anything back: the launch count is fixed (props 2, the
 * others 1), so a captured hipGraph replays them.  Integers only up to acc, table, count and dropped: two runs are
 * bit-identical, whatever order workgroups ran in.  n <= 65535; 1 <= nl <= 256; h, w <= ISA_PROPS_MAX_SIDE (so that no sum
 * can pass 2^63).  x is the column and y the row of a pixel.
 * isa_label_props: labels uint8 [n,h,w] (4-byte aligned, h*w % 4 == 0; 16-byte aligned maps with h*w % 16 == 0 are read 16
 *   pixels per load); image uint8 [n,h,w,c], c in {1,3,4} (c == 4: 4-byte aligned), or NULL with c == 0.
 *   acc int64 [n][nl][ISA_PROPS_ACC] (8-byte aligned), set to the empty values by the entry itself; oob int32 [n] counts
 *   the pixels with label >= nl (cleared by the entry).  Label 0 is background and is not measured: its row stays empty.
 *   Slots of label v (empty label):  0 area (0);  1, 2 min x, max x (w, -1);  3, 4 min y, max y (h, -1);
 *     5, 6 sum x, sum y (0);  7, 8, 9 sum x^2, sum y^2, sum x*y (0);  10 perimeter (0);
 *     11 smallest row-major pixel index y*w + x (h*w);  12..15 sum of image channel 0..3 (0; absent channels 0).
 *   Perimeter is the crack length: the number of (pixel, 4-neighbour) pairs where the pixel holds v and the neighbour
 *   holds another value or lies outside the image.  One pixel: 4; a 2 x 3 rectangle: 10; the edges of a hole count.
 * isa_instance_props: out double [n][nl][ISA_PROPS_OUT] (8-byte aligned) from acc; c as given to isa_label_props.
 *     0 area          1..4 half-open box x0, y0, x1, y1 (min, min, max + 1, max + 1)          5, 6 centroid sum x / A, sum y / A
 *     7, 8, 9 central second moments per pixel mxx = (A sum x^2 - (sum x)^2) / A^2, myy, mxy = (A sum xy - sum x sum y) / A^2:
 *       the numerators are formed exactly in 128-bit integers, then divided once
 *     10, 11 major and minor axis length 4 sqrt(l1), 4 sqrt(l2), l1,2 = (mxx + myy) / 2 +- sqrt(((mxx - myy) / 2)^2 + mxy^2)
 *     12 eccentricity sqrt(1 - l2 / l1), 0 when l1 == 0
 *     13 orientation 0.5 atan2(2 mxy, mxx - myy) in (-pi/2, pi/2], 0 when both arguments are 0: the angle of the major axis
 *        from the x axis, positive towards +y, and y points DOWN (rows), so a positive angle turns clockwise on the screen.
 *        This is the project's own convention (not scikit-image's, which measures from the row axis).
 *     14 perimeter          15 1.0 if the box touches an image edge, else 0.0          16 extent A / box area
 *     17 equivalent diameter sqrt(4 A / pi)          18 compactness 4 pi A / P^2          19 first pixel index
 *     20..23 mean of image channel 0..3, NaN for absent channels
 *   A label with area 0 (label 0 always) gives column 0 = 0 and NaN everywhere else.
 * isa_props_select: table uint8 [n][256] (old label -> new label), count int32 [n], dropped int32 [n] from acc.  A label
 *   1..nl-1 survives when it is non-empty, min_area <= area, area <= max_area (max_area == 0: no upper limit) and, with
 *   clear_border == 1, its box touches no image edge.  The survivors are ranked by `order` - ISA_ORDER_LABEL: old label
 *   ascending; ISA_ORDER_AREA: area descending, equal areas by the smaller old label; ISA_ORDER_RASTER: first pixel
 *   ascending - and the first max_objects (1..255) get the new labels 1, 2, ..; every other entry of the table is 0.
 *   count = labels given, dropped = non-empty labels - count.
 * isa_relabel_u8: out[i][p] = table[i][labels[i][p]] for uint8 maps [n, L]; L % 4 == 0, L < 2^31, maps 4-byte aligned
 *   (16-byte accesses when both are 16-byte aligned and L % 16 == 0).  out == labels is allowed; any other overlap is
 *   ISA_EINVAL. */
#define ISA_PROPS_ACC 16
#define ISA_PROPS_OUT 24
#define ISA_PROPS_MAX_SIDE 32768
enum { ISA_ORDER_LABEL = 0, ISA_ORDER_AREA = 1, ISA_ORDER_RASTER = 2 };
int isa_label_props(const uint8_t* labels, const uint8_t* image, int32_t n, int32_t h, int32_t w, int32_t c, int32_t nl,
                    int64_t* acc, int32_t* oob, void* stream);
int isa_instance_props(const int64_t* acc, int32_t n, int32_t nl, int32_t h, int32_t w, int32_t c, double* out,
                       void* stream);
int isa_props_select(const int64_t* acc, int32_t n, int32_t nl, int32_t h, int32_t w, int32_t min_area, int32_t max_area,
                     int32_t clear_border, int32_t order, int32_t max_objects, uint8_t* table, int32_t* count,
                     int32_t* dropped, void* stream);
int isa_relabel_u8(const uint8_t* labels, const uint8_t* table, int32_t n, int64_t L, uint8_t* out, void* stream);
/* ---- tracing instance outlines: polygons, holes, Euler number -----------------------------------------------------------
 * Both entries check every argument before they launch or write anything (ISA_EINVAL, then ISA_ENOMEM, then ISA_EALIGN),
 * are asynchronous on `stream`, allocate nothing and never read anything back: the launch count depends on the shape alone
 * (trace: 2 R + 9 with R = ceil(log4(4 h w)), the pointer-jumping rounds, taken from the edge bound and never from the data;
 * topology: 1), so a captured hipGraph replays them.  Only integers decide anything and every scattered write goes to a
 * slot one thread owns: two runs are bit-identical, whatever order workgroups ran in.  n <= 65535.
 * Definitions.  Pixel (row y, column x) is the unit square with corners (x, y) and (x+1, y+1); y points down.  For a pixel
 *   of label v != 0 every side whose 4-neighbour holds another value, or lies outside the image, is one directed unit EDGE
 *   of label v with the pixel on its right: top (x,y)->(x+1,y), direction E = 0; right (x+1,y)->(x+1,y+1), S = 1; bottom
 *   (x+1,y+1)->(x,y+1), W = 2; left (x,y+1)->(x,y), N = 3.  One pixel alone is the cycle E, S, W, N, clockwise on the
 *   screen.  The edges of v number the crack perimeter of isa_label_props.  An edge's KEY is
 *   (y0 * (w + 1) + x0) * 4 + direction, (x0, y0) its start point.
 *   Successor: an edge of label v and direction d ends at P; of the two pixels ahead of P let R say whether the one on the
 *   right holds v and L whether the one on the left does.  Connectivity 8: turn left (d - 1) if L, else straight if R,
 *   else right (d + 1).  Connectivity 4: turn right if not R, else left if L, else straight.  Every edge has exactly one
 *   successor and one predecessor of its own label; the edges fall into disjoint cycles, and a cycle is a CONTOUR.
 *   A CORNER EDGE is an edge whose predecessor has another direction.  The vertices of a contour are the start points of
 *   its corner edges in cycle order, the first one that of the corner edge with the smallest key, the contour's START KEY.
 *   Twice-area = sum(x_i * y_{i+1} - x_{i+1} * y_i) over the vertices: positive for an outer contour, negative for a hole;
 *   over the contours of a label it sums to twice the label's pixel count.  The outer contours of v are its connected
 *   components under the connectivity, its holes the enclosed components of "not v" under the dual one; Euler number =
 *   outer - holes.
 * isa_contour_trace: labels uint8 [n,h,w] (4-byte aligned), w % 4 == 0, h and w <= ISA_CONTOUR_MAX_SIDE; connectivity 4
 *   or 8; cmax >= 1, vmax >= 1.
 *   table int64 [n][cmax][8] (8-byte aligned), the contours of an image in ascending order of start key:
 *     0 label   1 offset of the first vertex in the image's verts   2 vertex count   3 edge count (crack length)
 *     4 signed twice-area   5 start key   6 row-major index of the pixel that owns the start edge   7 always 0
 *   verts int16 [n][vmax][2] (4-byte aligned): (x, y), the vertices of contour 0 first, then those of contour 1, ...
 *   counts int32 [n][4] (4-byte aligned): contours found, vertices found (both whatever the capacities),
 *     contours beyond cmax = max(0, [0] - cmax), vertices beyond vmax = max(0, [1] - vmax).
 *   Overflow: the first cmax contours get their rows, offsets counted over ALL vertices before them; the vertices of a
 *   contour are written only when it has a row and offset + count <= vmax, so what is written is a prefix.  Rows and
 *   vertices past that keep what the caller left there; nothing is written outside the buffers.
 *   scratch: ISA_CONTOUR_SCRATCH_BYTES(n,h,w) bytes, 16-byte aligned, need not be cleared: per image 48 bytes for each of
 *   the ISA_CONTOUR_EDGES = 4 h w possible edges (two 16-byte jumping records, key, successor, corner flag, start
 *   edge), 4 per lattice point (index of its first edge) and the block sums of the two scans.
 * isa_contour_topology: topo int32 [n][nl][3] (4-byte aligned; 1 <= nl <= 256), set by the entry itself: outer contours
 *   (= components), holes and Euler number of label v, from the min(counts[i][0], cmax) rows the table holds (contours
 *   beyond cmax are not in it: the caller sees that from counts); rows of a label >= nl are skipped, label 0 is all 0. */
#define ISA_CONTOUR_MAX_SIDE 4096
#define ISA_CONTOUR_BLOCK 1024
#define ISA_CONTOUR_EDGES(h, w) ((int64_t)4 * (h) * (w))
#define ISA_CONTOUR_POINTS(h, w) ((((int64_t)(h) + 1) * ((int64_t)(w) + 1) + 3) / 4 * 4)
#define ISA_CONTOUR_SCRATCH_BYTES(n, h, w)                                                                     \
    ((int64_t)(n) * (ISA_CONTOUR_EDGES(h, w) * 48 + ISA_CONTOUR_POINTS(h, w) * 4 +                             \
                     (ISA_CONTOUR_POINTS(h, w) / ISA_CONTOUR_BLOCK + 1) * 16 +                                 \
                     (ISA_CONTOUR_EDGES(h, w) / ISA_CONTOUR_BLOCK + 1) * 16 + 16))
int isa_contour_trace(const uint8_t* labels, int32_t n, int32_t h, int32_t w, int32_t connectivity, int32_t cmax,
                      int32_t vmax, int64_t* table, int16_t* verts, int32_t* counts, void* scratch, int64_t scratch_bytes,
                      void* stream);
int isa_contour_topology(const int64_t* table, const int32_t* counts, int32_t n, int32_t cmax, int32_t nl, int32_t* topo,
                         void* stream);
/* ---- exact Euclidean distance transform to the two nearest instances; border weights and instance fill -----------------
 * Every entry checks all its arguments before it launches or writes anything (ISA_EINVAL / ISA_EALIGN / ISA_ENOMEM), is
 * asynchronous on `stream`, allocates nothing and never reads anything back: the launch count depends on the shape alone,
 * so a captured hipGraph replays them.  Only integers decide anything in the transform and the fill: the results are
 * unique, and two runs are bit-identical.
 * isa_edt2_u8: labels uint8 [n,h,w] (4-byte aligned), 0 = no instance; n <= 65535, h and w <= ISA_EDT_MAX_SIDE, w % 4 == 0.
 *   With D_k(p) the squared Euclidean distance (an integer) from pixel p to the nearest pixel of its image that holds label
 *   k, over the labels present in that image (D_k = 0 on a pixel of label k):
 *     d1sq int32 [n,h,w] (16-byte aligned): the smallest D_k; INT32_MAX when the image holds no label.
 *     d2sq int32 [n,h,w] (16-byte aligned): the second smallest D_k as a multiset (= d1sq when two labels tie); INT32_MAX
 *       when the image holds fewer than two labels.
 *     nearest uint8 [n,h,w] (4-byte aligned): the smallest label k with D_k = d1sq; 0 when the image holds no label.
 *   Any of the three may be NULL.  scratch: ISA_EDT_SCRATCH_BYTES(n,h,w) bytes, 16-byte aligned, need not be cleared (two
 *   packed (vertical distance, label) entries per pixel).  Two launches: one lane per column (ISA_EDT_COL_LANES columns
 *   per workgroup) sweeps it down and up; one workgroup of min(ISA_EDT_ROW_LANES, w rounded up to 64) lanes per row walks
 *   outwards from every pixel over the row's entries in LDS (8 w + 16 bytes) until nothing farther can matter.
 * isa_border_weights: out fp32 [n,hw] (16-byte aligned) = 1 where labels != 0 or d2sq is INT32_MAX, else
 *   1 + w0 * expf(-(sqrtf(d1sq) + sqrtf(d2sq))^2 / (2 sigma^2)).  cfg: device float[2] = {w0, sigma}, read at run time, so a
 *   captured hipGraph follows in-place changes.  hw % 4 == 0, hw < 2^30; one launch.
 * isa_fill_labels: out uint8 [n,hw] (4-byte aligned; it must not overlap labels: ISA_EINVAL) = labels where that is
 *   non-zero; else nearest where fg != 0 and d1sq <= max_dist_sq (max_dist_sq < 0: no limit); else 0.  filled int32 [n]:
 *   pixels filled per image (cleared by the entry, integer adds).  labels, fg, nearest 4-byte aligned, d1sq 16-byte
 *   aligned, hw % 4 == 0, n <= 65535; two launches. */
#define ISA_EDT_MAX_SIDE 4096
#define ISA_EDT_COL_LANES 64
#define ISA_EDT_ROW_LANES 256
#define ISA_EDT_SCRATCH_BYTES(n, h, w) ((int64_t)(n) * (h) * (w) * 8)
int isa_edt2_u8(const uint8_t* labels, int32_t n, int32_t h, int32_t w, int32_t* d1sq, int32_t* d2sq, uint8_t* nearest,
                void* scratch, int64_t scratch_bytes, void* stream);
int isa_border_weights(const uint8_t* labels, const int32_t* d1sq, const int32_t* d2sq, const float* cfg, int32_t n,
                       int64_t hw, float* out, void* stream);
int isa_fill_labels(const uint8_t* labels, const uint8_t* fg, const uint8_t* nearest, const int32_t* d1sq,
                    int32_t max_dist_sq, int32_t n, int64_t hw, uint8_t* out, int32_t* filled, void* stream);
int isa_ins_softmax_bwd(const float* alpha, const int64_t* ins, const int32_t* idx, const int32_t* s_t,
                        const float* adv, int32_t n, int32_t nobj, int64_t L, float* dmerge /*[nsrc, L]*/, int32_t nsrc,
                        void* stream);
int isa_maskbn_bwd(const isa_tensor* e, const float* sem, const float* dmerge, const float* mean_var,
                   const float* w, float eps, const float* am, int32_t train, float* red4 /*zeroed*/, float* k2,
                   float* dw, float* db, const isa_tensor* de, int32_t accumulate, void* stream);
int isa_sp_bwd(const isa_tensor* dout, const isa_tensor* x, const float* beta, const float* m, const float* dot,
               const float* rowstat, const float* chansum, const float* scale, const float* mean,
               const float* invstd, const float* wv, const float* lh, const float* fcw, float count, int32_t train,
               float* scratch /*zeroed: 3C + 2*rup(n,4) + 2*n*L floats*/, const isa_tensor* dx, int32_t accumulate,
               float* d_gamma, float* d_beta, float* d_wv, float* d_bv, float* d_lh, float* d_fcw, float* d_fcb,
               void* stream);
int isa_gate_bwd(const isa_tensor* dout, const isa_tensor* up, const float* gmap, const isa_tensor* dup,
                 int32_t acc_up, float* du /*zeroed [n*H*W]*/, const isa_tensor* dpred, int32_t acc_pred, void* stream);
int isa_se_bwd(const isa_tensor* dxa, const isa_tensor* x, const float* gate, const float* hid, const float* mean,
               const float* w1, const float* w2, int32_t hidden, float* dg /*zeroed [n*c]*/, float* dmean /*[n*c]*/,
               float* dw1, float* db1, float* dw2, float* db2, const isa_tensor* dx, int32_t accumulate, void* stream);
/* dst (+)= src * s[n,c]  (Dropout2d backward on a residual sum).  src may hold G * dst.n images (a tensor that was
 * broadcast to G statistic groups, each with its own per-image scale): dst[b] (+)= sum_g src[g*n+b] * s[g*n+b]. */
int isa_scale_bc(const isa_tensor* src, const float* s_bc, const isa_tensor* dst, int32_t accumulate, void* stream);
/* optimizer on the flat parameter buffer (model.py:145-166,273-278): out += sum (g*scale)^2, then
 * clip_grad_norm_(max_norm) + Adadelta(lr, rho, eps, weight_decay) in one pass.  lr_dev (optional, device float[1])
 * overrides `lr` at run time, so a launch recorded in a hipGraph follows the scheduler (model.py:164,437). */
int isa_sqnorm(const float* g, int64_t n, float scale, float* out /*zeroed*/, void* stream);
int isa_adadelta(float* p, const float* g, float* sq, float* acc, int64_t n, float lr, float rho, float eps, float wd,
                 const float* sqnorm, float max_norm, float gscale, const float* lr_dev, void* stream);
/* The other optimizers model.py:145-166 accepts, with the semantics of torch.optim.{Adam, RMSprop, SGD} as constructed
 * there (L2 weight decay added to the gradient; no amsgrad, no RMSprop momentum or centring, SGD dampening 0 and no
 * Nesterov), fused with the clip exactly like isa_adadelta: gr = g*gscale*clip + wd*p, state update, parameter write,
 * clip = min(1, max_norm / (sqrt(sqnorm[0]) + 1e-6)) when max_norm > 0; lr_dev as above.  One streaming launch over n
 * floats each; p, g and the state ranges must be 16-byte aligned (ISA_EALIGN), state starts zeroed.  Decay rates are
 * doubles so that 1 - beta is rounded once, as torch rounds it.
 * isa_adam: `step` (device int32[1], starts 0) counts the updates in device memory - a one-thread launch ahead of the
 * update increments it and writes aux (device float[4], 16-byte aligned) = {gscale*clip, 1 - beta1^step, 1 - beta2^step,
 * sqrt(1 - beta2^step)}, which the update reads - so a launch recorded in a hipGraph keeps its bias correction exact. */
int isa_adam(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int32_t* step, float* aux, int64_t n, float lr,
             double beta1, double beta2, float eps, float wd, const float* sqnorm, float max_norm, float gscale,
             const float* lr_dev, void* stream);
int isa_rmsprop(float* p, const float* g, float* square_avg, int64_t n, float lr, double alpha, float eps, float wd,
                const float* sqnorm, float max_norm, float gscale, const float* lr_dev, void* stream);
int isa_sgd(float* p, const float* g, float* momentum_buffer, int64_t n, float lr, double momentum, float wd,
            const float* sqnorm, float max_norm, float gscale, const float* lr_dev, void* stream);

/* ---- the reference's named attention operators (modules/utils.py; dead at HEAD) --
 * a19 ScaledDotProductAttention.forward (utils.py:316-327) as MultiHeadAttention calls it (utils.py:167-225):
 *     out = softmax(mask(q k^T / T)) v, attn[(head*b), lq, L] optional (fp32).  Few queries against L = H*W keys.
 *     Operands: k, v [bh, L, heads*d], q [bh, lq, heads*d], out [bh, lq, heads*d] with `heads` heads interleaved in a
 *     row - the layout the Linear projections produce, so the reference's head-major permute (utils.py:200-202) is
 *     never materialised; heads = 1 means plain contiguous [bh, L, d] operands (then bh = batch*heads).
 *     dtype ISA_F32 | ISA_BF16 | ISA_F16.  mask: bytes, non-zero = masked, [bh, lq, L] or, with mask_per_head,
 *     [heads*bh, lq, L] (the reference repeats the mask per head).  attn rows are ordered head-major ((h*bh + b)*lq + q)
 *     like the reference's (n*b) batch.
 *     d_k = d_v = 12 (config.py:22-25): split-L streaming kernel - K/V read once in 16-byte coalesced loads, LDS-staged
 *     tiles of `tile_keys` keys (0 = 512; 256/512/1024), lane = key, online softmax, shuffle merges, one partial per
 *     workgroup in `ws` and a flash-decoding merge.  Other head dims <= 32: a one-workgroup-per-query fallback
 *     (heads = 1, f32/bf16).  ws: fp32 scratch, bh*heads*lq*(nsplit*(2+d)+2) floats (64 K floats always suffice). */
int isa_sdp_attention(const void* q, const void* k, const void* v, const uint8_t* mask, void* out,
                      float* attn, int32_t bh, int32_t lq, int64_t L, int32_t dk, int32_t dv,
                      float temperature, int32_t dtype, int32_t heads, int32_t mask_per_head,
                      float* ws, int64_t ws_floats, int32_t tile_keys, void* stream);
/* Backward of isa_sdp_attention (what autograd computes for utils.py:316-327 with dropout off), from the tensors the
 * forward pass returns: attn (normalised probabilities, head-major rows, zero on masked keys) and out.  dq: fp32
 * [bh, lq, heads*d], ZERO-INITIALISED by the caller (partials are added atomically); dk, dv: storage dtype, same layout
 * as k, v, written once.  One streaming pass over K and V.  lq <= 8, d <= 32, lq*d <= 96.  `bh` is the batch (rows of
 * q), `heads` the interleaved heads per row, exactly as in the forward call. */
int isa_sdp_attention_bwd(const void* q, const void* k, const void* v, const float* attn, const void* out,
                          const void* dout, float* dq, void* dk, void* dv, int32_t bh, int32_t lq, int64_t L,
                          int32_t dk_dim, int32_t dv_dim, float temperature, int32_t dtype, int32_t heads, void* stream);
/* The `last=True` branch (utils.py:203-209, 310-313): out[(h*b), lq, L] = q k^T (ScaledDotProductAttention) or
 * sigmoid(q k^T) (MultiHeadAttention: sigmoid != 0), no temperature, no softmax; same operand layout. */
int isa_sdp_scores(const void* q, const void* k, float* out, int32_t b, int32_t heads, int32_t lq, int64_t L,
                   int32_t d, int32_t dtype, int32_t sigmoid, void* stream);
/* y[r,:] = LayerNorm(W x[r,:] + bias + residual[r,:]): the small dense layers around the attention core (w_qs on the few
 * query rows, fc + layer_norm on the attended rows, utils.py:189-201).  fp32, n <= 64; gamma == NULL: no LayerNorm. */
int isa_linear_ln(const float* x, const float* w, const float* bias, const float* residual, const float* gamma,
                  const float* beta, float eps, int32_t rows, int32_t k, int32_t n, float* y, void* stream);
/* out = InstanceNorm2d(x + res) (utils.py:301-302: affine=False, biased variance); sums: zeroed float[n][2c].
 * x, res, out: the same n, h, w, c (c <= 64) and dtype.  Two statistics passes over the values minus the (image,
 * channel)'s first one: sums[b][0..c) receives their sum, sums[b][c..2c) the sum of their squared distances from their
 * mean, so a channel offset costs no digits of the variance. */
int isa_instance_norm_res(const isa_tensor* x, const isa_tensor* res, const isa_tensor* out, float eps, float* sums,
                          void* stream);
/* a20 _ScalePDAttention core (utils.py:276-299): per-pixel softmax over the 3x3 neighbourhood at `dilation`.
 * q, k [n,h,w,dk], v, out [n,h,w,dv] (the same n, h, w and dtype; dk, dv <= 32); nomask: fp32 [n, h*w], values in
 * {0, 1}, non-zero = masked key.  `scale` multiplies the logits <q, k>; finite and > 0.  The reference's is c^-1/2 with
 * c the per-head INPUT width d_model / n_head (utils.py:273,293: `c` is read off qk after the head view), which equals
 * d_k^-1/2 only where d_model / n_head == d_k. */
int isa_local_attention(const isa_tensor* q, const isa_tensor* k, const isa_tensor* v, const float* nomask,
                        const isa_tensor* out, int32_t dilation, float scale, void* stream);
/* a21 Decoder.forward (utils.py:59-69): out[b,p] = sigmoid(<q[b,:], enc[b,p,:]>) */
int isa_point_query(const float* q, const isa_tensor* enc, float* out, void* stream);

/* ---- input expansion: ImageEx + ToTensor + Standardization, code/lib/utils.py:90-113 and
 * code/lib/preprocess.py:192-195.  rgb: uint8 [n,h,w,3] (device); out: NHWC view with c == 21 (ld 24: the three pad
 * channels are written as zero).  out = ([rgb, lab, hsv, yuv, ycbcr, hed, yiq] - 0.5) * 2.                     */
int isa_image_ex(const uint8_t* rgb, const isa_tensor* out, void* stream);

/* ---- target expansion (the tail of the collate function): AlignCollate.__call__,
 * code/lib/dataset.py:349-379, widens the uint8 instance planes to int64 [bs,K,h,w] and builds the int64 semantic
 * one-hot [bs,2,h,w] on the host.  Here: ins uint8 [n,h,w,k] (the array `instance_annotations` of :349-351 before
 * the cast) -> ins_out int64 [n,k,h,w], values preserved; sem uint8 [n,h,w] (may be NULL) -> sem_out int64 [n,2,h,w],
 * channel c = (sem == c) as np.eye(2)[sem] (:356-361; a value > 1 is an IndexError there and all-zero here).  k <= 252. */
int isa_collate_targets(const uint8_t* ins, const uint8_t* sem, int32_t n, int32_t h, int32_t w, int32_t k,
                        int64_t* ins_out, int64_t* sem_out, void* stream);
/* isa_collate_targets with a K-class semantic one-hot: sem_out int64 [n,n_classes,h,w] = np.eye(n_classes)[sem]
 * (dataset.py:365-369), 2 <= n_classes <= ISA_SEM_MAX_CLASSES; labels_out (may be NULL) uint8 [n,h,w], a copy of sem for
 * the K-class criterion.  sem_out may be NULL when labels_out is given. */
int isa_collate_targets_k(const uint8_t* ins, const uint8_t* sem, int32_t n, int32_t h, int32_t w, int32_t k,
                          int32_t n_classes, int64_t* ins_out, int64_t* sem_out, uint8_t* labels_out, void* stream);

/* ---- exact augmentations: the index-permuting part of AlignCollate.__preprocess,
 * code/lib/dataset.py:185-233 - horizontal flip, vertical flip, transpose, rotation by k*90 degrees (preprocess.py:171,
 * 218,286,323; PIL FLIP_LEFT_RIGHT / FLIP_TOP_BOTTOM / TRANSPOSE / rotate(expand=True)), in the reference's order.
 * src: uint8 [n,h,w,c] (c = 3 image, 1 semantic map, 32 instance planes), out of place; dst: [n,h,w,c], or [n,w,h,c] when
 * swap_axes != 0 - an op that transposes XOR turns an odd number of quarters exchanges the axes, so one call covers the
 * images whose ops agree in that parity (any mix on square images).  The reference augments the original, non-square
 * image (e.g. 2362 x 672) before the resize.
 * ops_dev: int32 [n] on the device, per image: bit0 hflip, bit1 vflip, bit2 transpose, bits 3-4 = quarter turns
 * counter-clockwise (rot_angle / 90).  The random draws stay on the host as in the reference (:186,198,210,222). */
int isa_d4_augment(const uint8_t* src, uint8_t* dst, int32_t n, int32_t h, int32_t w, int32_t c, int32_t swap_axes,
                   const int32_t* ops_dev, void* stream);

/* ---- the non-D4 augmentations the reference ships enabled (settings/CVPPP/training_settings.py:40 ROTATION, :50
 * CENTER_CUT), AlignCollate.__preprocess code/lib/dataset.py:236-269 ------------------------------------------------
 * Rotation by `angle` degrees (an integer in [-9, 9], dataset.py:237-239) with expand=True.  The geometry - output size
 * and the six affine coefficients - is Image.rotate's own Python float arithmetic and stays on the host
 * (isa_amd.data.rotate_geometry); h, w are the expanded output dims.
 * nearest (annotation planes and semantic map, preprocess.py:311-327 Image.NEAREST): Pillow's Geometry.c affine_fixed,
 *   coef = the six 16.16 fixed-point values {a0,a1,a2,a3,a4,a5} (HOST array), zero fill; any channel count.
 * bilinear (the RGB image, preprocess.py:330-365 rotate_with_random_bg): ImagingGenericTransform + bilinear_filter32RGB
 *   in IEEE double, (UINT8) truncation; pixels whose sample point lies outside the source take bg (HOST array, c bytes:
 *   the drawn background colour - white, black, int(mean) or int(median) of the source); c <= 4.
 * Both are bit-identical to the installed Pillow through oracle/rotate_ref.py (tests/test_oracle_rotate.py). */
int isa_rotate_nearest_u8(const uint8_t* src, int32_t n, int32_t h0, int32_t w0, int32_t c, uint8_t* dst, int32_t h,
                          int32_t w, const int32_t* coef_host, void* stream);
int isa_rotate_bilinear_u8(const uint8_t* src, int32_t n, int32_t h0, int32_t w0, int32_t c, uint8_t* dst, int32_t h,
                           int32_t w, const double* matrix_host, const uint8_t* bg_host, void* stream);
/* CenterCut (preprocess.py:239-264, dataset.py:252-269).
 * cover_rows: single[n,h,w] = 1 where exactly one instance plane covers the pixel (`ins_all == 1`, the candidate
 *   centres in row-major order), row_counts[n,h] = their number per row - the host picks the drawn candidate from h ints
 *   and one row of `single` instead of downloading the planes.
 * plane_sums: sums[n,c] (zeroed by the caller) += the sum of every channel over the window [y0,y0+h) x [x0,x0+w): the
 *   reference keeps a plane when its window sums to more than 30.
 * crop_planes: dst[n,h,w,cd] = the window of the channels chan_dev[j] (device int32 [cd]; -1 or out of range = a zero
 *   plane, NULL = identity): crop, compaction of the surviving planes and the zero planes up to 32 (dataset.py:304-311)
 *   in one pass; with c = cd = 3 / 1 the image and semantic-map crops. */
int isa_cover_rows_u8(const uint8_t* planes, int32_t n, int32_t h, int32_t w, int32_t k, uint8_t* single,
                      int32_t* row_counts, void* stream);
int isa_plane_sums_u8(const uint8_t* src, int32_t n, int32_t H, int32_t W, int32_t c, int32_t y0, int32_t x0, int32_t h,
                      int32_t w, int64_t* sums, void* stream);
int isa_crop_planes_u8(const uint8_t* src, int32_t n, int32_t H, int32_t W, int32_t c, int32_t y0, int32_t x0, uint8_t* dst,
                       int32_t h, int32_t w, int32_t cd, const int32_t* chan_dev, void* stream);

/* Nearest-neighbour resize of annotation planes: the `ann_resizer` of AlignCollate
 * (code/lib/dataset.py:162,168,293-320 -> utils.py:26-27 -> PIL Image.resize(NEAREST), once per instance plane and
 * semantic map on the host).  src uint8 [n,h0,w0,c] -> dst uint8 [n,h,w,c], out of place; source row/column tables
 * follow Pillow's ImagingScaleAffine exactly (half-step start, step accumulated in double), h, w <= 768.          */
int isa_resize_nearest_u8(const uint8_t* src, int32_t n, int32_t h0, int32_t w0, int32_t c, uint8_t* dst,
                          int32_t h, int32_t w, void* stream);

/* Bilinear image resize: the `img_resizer` of AlignCollate and Prediction (code/lib/dataset.py:160-161,
 * 166-167, prediction.py:37 -> utils.py:26-27 -> PIL Image.resize(BILINEAR)) for uint8 images [n,h0,w0,c] (c <= 4) ->
 * [n,h,w,c], bit-identical to Pillow's Resample.c (anti-aliased triangle filter, 22-bit fixed-point coefficients,
 * horizontal pass into a uint8 intermediate, then vertical).  ws: device scratch of isa_resize_bilinear_ws_bytes(...)
 * bytes (coefficient tables + the intermediate image); ISA_ENOMEM when smaller. */
int64_t isa_resize_bilinear_ws_bytes(int32_t n, int32_t h0, int32_t w0, int32_t c, int32_t h, int32_t w);
int isa_resize_bilinear_u8(const uint8_t* src, int32_t n, int32_t h0, int32_t w0, int32_t c, uint8_t* dst,
                           int32_t h, int32_t w, void* ws, int64_t ws_bytes, void* stream);

/* Lanczos image resize: the two `img.resize(size, Image.ANTIALIAS)` of the reference's random_resolution
 * (code/lib/preprocess.py:443-454; ANTIALIAS was Pillow's name for LANCZOS = 1) for uint8 [n,h0,w0,c] (c <= 4) ->
 * [n,h,w,c], out of place, bit-identical to Pillow: the same Resample.c passes as the bilinear entry with the filter
 * sinc(x) * sinc(x/3), support 3.  The coefficient tables are computed on the HOST inside the call, in IEEE double with
 * libm's sin (the device's sin may differ from it in the last bit, which now and then flips a 22-bit rounding), copied
 * into ws on the stream, and the call returns only once that copy has been made.  ws: device scratch of the *bytes that
 * isa_resize_lanczos_ws_bytes reports (a status like every entry but the bilinear one's; ISA_EINVAL for sizes the
 * resize would refuse), 4-byte aligned; ISA_ENOMEM when smaller.  Every size at most 65535. */
int isa_resize_lanczos_ws_bytes(int32_t n, int32_t h0, int32_t w0, int32_t c, int32_t h, int32_t w, int64_t* bytes);
int isa_resize_lanczos_u8(const uint8_t* src, int32_t n, int32_t h0, int32_t w0, int32_t c, uint8_t* dst,
                          int32_t h, int32_t w, void* ws, int64_t ws_bytes, void* stream);

/* ---- photometric augmentations: the four of AlignCollate.__preprocess that work pixel by pixel
 * (code/lib/dataset.py:147-155,271-281), which the reference runs as up to seven PIL passes per image:
 *   colour jitter  utils.py:58-59 -> torchvision ColorJitter(0.4, 0.4, 0.4, 0.2): ImageEnhance.Brightness / Contrast /
 *                  Color and the HSV hue shift, in a drawn order
 *   gamma          preprocess.py:405-439 Image.point over a 256-entry table
 *   channel swap   preprocess.py:381-401 img_np[:, :, np.random.choice([0, 1, 2], 3, True)]
 *   grayscale      utils.py:62-63 -> RandomGrayscale: convert('L') copied to three channels
 * Here one pass: every pixel is read once, taken through its image's program in registers - jitter ops in the listed
 * order -> LUT -> channel map -> grayscale, each stage rounding to uint8 exactly where Pillow holds a uint8 image - and
 * written once.  Bit-identical to the installed Pillow (tests/photometric_np.py, tests/test_photometric_ref.py).
 *   brightness  blend(0, x, f);  contrast  blend(m, x, f), m = int(mean(L) + 0.5) of the image as it stands when the op
 *   is applied;  saturation  blend(L, x, f);  blend(d, x, f) = float32 d + f * (x - d), clipped to [0, 255], truncated;
 *   L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
 *   hue  RGB -> HSV (Pillow's mix of float and double), H += hue_shift mod 256, HSV -> RGB.  The caller computes
 *   hue_shift = int(hue_factor * 255) & 255.  For hue_factor >= 0 that is numpy's `np_h += np.uint8(hue_factor * 255)`
 *   of torchvision's PIL path; the uint8 cast of a NEGATIVE float is platform-defined in numpy, so for those this
 *   definition (two's-complement wrap) is this library's own.
 * A program lists each op at most once; op[k] outside the four codes is skipped, chan[] entries above 2 read as 2. */
#define ISA_PHOTO_BRIGHTNESS 0
#define ISA_PHOTO_CONTRAST   1
#define ISA_PHOTO_SATURATION 2
#define ISA_PHOTO_HUE        3
typedef struct {
    int32_t n_ops;        /* 0..4 jitter ops, applied in the order op[0], op[1], ... */
    uint8_t op[4];        /* ISA_PHOTO_* */
    float factor[4];      /* blend factor of op[k] (unused for hue) */
    uint8_t hue_shift;    /* added to H mod 256 */
    uint8_t use_lut;      /* != 0: every channel through lut[] (gamma) */
    uint8_t gray;         /* != 0: L of the result to all three channels */
    uint8_t chan[3];      /* output channel c takes channel chan[c]; duplicates allowed; {0,1,2} = none */
    uint8_t pad[2];
    uint8_t lut[256];
} isa_photo_prog;         /* 288 bytes */
/* src uint8 [n,h,w,3] -> dst uint8 [n,h,w,3]; src == dst is allowed (the pass is elementwise).  progs_dev: n programs
 * on the device, one per image.  has_contrast != 0: some program holds a contrast op; a pre-pass then sums L of those
 * images (after the ops listed before contrast) into sums_ws, device int64 [n], which the call zeroes itself.  With
 * has_contrast == 0 sums_ws may be NULL and a contrast op in a program is skipped.  n <= 65535. */
int isa_photometric_u8(const uint8_t* src, uint8_t* dst, int32_t n, int32_t h, int32_t w, const isa_photo_prog* progs_dev,
                       int32_t has_contrast, int64_t* sums_ws, void* stream);

/* ---- elastic deformation: a smooth random displacement field and the warp of uint8 tensors by a field ------------------
 * (Simard, Steinkraus & Platt 2003; the companion of the border weight map in Ronneberger et al. 2015.)  Both entries
 * check every argument before they launch or write anything (ISA_EINVAL / ISA_EALIGN / ISA_ENOMEM), are asynchronous on
 * `stream`, allocate nothing and never synchronise.  n in 1..65535, h and w in 1..ISA_WARP_MAX_SIDE.
 * isa_elastic_field: noise fp32 [n,h,w,2] (8-byte aligned) with values in [-1, 1) ->
 *     disp[b,y,x,k] = alpha_dev[b] * G(noise)[b,y,x,k]      (fp32 [n,h,w,2], 8-byte aligned; it must not overlap noise)
 *   G is a separable Gaussian blur along x and then along y with zeros outside the image (scipy's mode='constant', cval=0).
 *   Component 0 is dx (along columns), component 1 is dy (along rows).  taps_host: the 2*radius+1 fp32 weights, on the HOST;
 *   the call reads them before it returns and hands them to the kernels by value.  radius in 0..ISA_ELASTIC_MAX_RADIUS;
 *   radius == 0: disp = alpha * noise.  alpha_dev: device fp32 [n], 4-byte aligned; an image with alpha 0 gets an all-zero
 *   field.
 *   scratch: ISA_ELASTIC_SCRATCH_BYTES(n,h,w) bytes, 16-byte aligned, need not be cleared, apart from noise and disp.
 *   Two launches: one workgroup per image row (the row and its zeroed halo in LDS), then one workgroup per 64 columns x
 *   32 rows that slides over the rows it taps in 32-row LDS chunks and scales by alpha.  fp32, taps added in ascending
 *   order, no atomics: two runs give the same bits.
 * isa_warp_u8: dst[b,y,x,:] = src uint8 [n,h,w,c] sampled at (x + disp[b,y,x,0], y + disp[b,y,x,1]), coordinates clamped to
 *   the image (replicate border).  c in 1..ISA_WARP_MAX_CHANNELS; src and dst 4-byte aligned, disp 8-byte aligned; dst may
 *   overlap neither src nor disp.  The arithmetic is integers after one rounding.  For each component d of disp:
 *     1. NaN becomes 0, then d is clamped to [-16384, 16384] (+-Inf end there);
 *     2. q = x * 256 + (int)rintf(d * 256.0f) in int32 (the product is exact, rintf rounds half to even); likewise for y;
 *     3. ISA_WARP_NEAREST: xs = clamp((qx + 128) >> 8, 0, w-1), likewise ys (arithmetic shifts); dst = src[ys, xs];
 *     4. ISA_WARP_BILINEAR: x0 = qx >> 8, fx = qx & 255, likewise y; taps (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1), every
 *        index clamped into the image on its own, weights (256-fx)(256-fy), fx(256-fy), (256-fx)fy, fx*fy;
 *        dst = (sum + 32768) >> 16.
 *   One launch: c == 32 a lane per pixel and 16-byte channel group, c <= 4 a lane per pixel, otherwise a lane per byte. */
#define ISA_ELASTIC_MAX_RADIUS 64
#define ISA_WARP_MAX_SIDE 1024
#define ISA_WARP_MAX_CHANNELS 64
#define ISA_WARP_NEAREST 0
#define ISA_WARP_BILINEAR 1
#define ISA_ELASTIC_SCRATCH_BYTES(n, h, w) ((int64_t)(n) * (h) * (w) * 8)
int isa_elastic_field(const float* noise, const float* alpha_dev, int32_t n, int32_t h, int32_t w,
                      const float* taps_host, int32_t radius, float* disp,
                      void* scratch, int64_t scratch_bytes, void* stream);
int isa_warp_u8(const uint8_t* src, const float* disp, int32_t n, int32_t h, int32_t w, int32_t c,
                int32_t mode, uint8_t* dst, void* stream);

/* ---- copy-paste augmentation (Ghiasi et al., CVPR 2021): instances of another image of the batch pasted over the target ----
 * One entry runs the whole stage on `stream`: the paste plan, the capacity limit, the occluded planes, the compaction of
 * the survivors and the new object counts, all on the device.  It allocates nothing, never synchronises and reads nothing
 * back; the launch sequence does not depend on the data (a launch that clears the scratch, then three), so the call can
 * be captured in a hipGraph.  Every argument is checked before anything is launched or written.
 * Inputs, device memory, a batch of n images of one size h x w:
 *   rgb uint8 [n,h,w,c], c in 1..4;  sem uint8 [n,h,w];
 *   planes uint8 [n,h,w,k], k in 1..ISA_PASTE_MAX_PLANES: the first n_objects[b] planes of image b are real.  Only "zero /
 *     non-zero" of a plane byte matters for decisions; byte values are carried through unchanged;
 *   n_objects int32 [n], clamped to 0..k by the kernels;
 *   xform int32 [n,4] = {src, flip, dy, dx} per target image;  select uint32 [n]: bit j = source plane j is a candidate;
 *   min_area by value; values < 1 mean 1.
 * For target image b with s = src; any s outside 0..n-1 means "no paste" (s == b is allowed):
 *  1. Geometry.  For a target pixel (y, x): u = x - dx, v = y - dy.  The pixel is IN FRAME iff 0 <= u < w and 0 <= v < h.
 *     The source pixel is xs = (flip & 1) ? w-1-u : u, ys = (flip & 2) ? h-1-v : v: the source is flipped, then shifted by
 *     (dy, dx).  Any int32 shift is legal; a shift that leaves nothing in frame pastes nothing.
 *  2. Areas.  area[j] = the number of in-frame target pixels whose source byte planes[s,ys,xs,j] is non-zero, for
 *     j < n_objects[s].  Planes at or beyond n_objects[s] are ignored even if they hold non-zero bytes.
 *  3. Paste set P.  Walk j ascending over j < n_objects[s]: j is a candidate iff bit j of select[b] is set and
 *     area[j] >= max(min_area, 1).  P is the first k - n_objects[b] candidates (the capacity rule: the count of target
 *     planes BEFORE occlusion bounds it, which keeps the rule non-circular).
 *  4. P empty: image b passes through.  rgb, sem and the planes 0..n_objects[b]-1 are copied byte for byte, the planes
 *     behind them are zero, n_out[b] = n_objects[b]; nothing is dropped, even an empty real plane.
 *  5. Otherwise M(y,x) = in frame and some j in P has a non-zero source byte.  Where M holds: rgb_out = rgb[s,ys,xs,:],
 *     sem_out = sem[s,ys,xs], every target plane byte becomes 0.  Elsewhere the outputs equal the target's inputs.
 *  6. Pasted planes.  For j in P: q_j(y,x) = planes[s,ys,xs,j] in frame, 0 outside.
 *  7. Survival and order.  A target plane i < n_objects[b] is kept iff it has a non-zero byte left after step 5.  Output
 *     planes: first the kept target planes in ascending i, then the pasted planes in ascending j, then zero planes up to k.
 *     n_out[b] = kept + |P|, at least 1 and at most k.
 *  8. plan int32 [n,4] = {pasted bits (over j), kept-target bits (over i), n_out, area-limited flag}.  The flag is 1 iff a
 *     plane j < n_objects[s] with its select bit set was refused by min_area or by capacity.  A pass-through image has
 *     pasted bits 0 and kept bits (1 << n_objects[b]) - 1; with s outside 0..n-1 the flag is 0.
 * No blending of the seam.  No output (rgb_out, sem_out, planes_out, n_out, plan, scratch) may overlap an input or another
 * output: ISA_EINVAL (another target may still read image b as its source).
 * Limits: n in 1..65535; h, w in 1..ISA_PASTE_MAX_SIDE.  Alignment (ISA_EALIGN): n_objects, xform, select, n_out, plan and
 * scratch 4 bytes; planes and planes_out 16 bytes when k % 16 == 0 (pixel vectors then move as 16-byte loads and stores),
 * 1 byte otherwise; rgb, sem and their outputs 1 byte.  scratch: ISA_COPY_PASTE_SCRATCH_BYTES(n, k) bytes (the int32 area
 * and remaining-area counters per image and plane), ISA_ENOMEM when smaller; it need not be cleared by the caller.
 * Counters are integer atomics and there is no float arithmetic: two runs give the same bytes. */
#define ISA_PASTE_MAX_SIDE 4096
#define ISA_PASTE_MAX_PLANES 32
#define ISA_COPY_PASTE_SCRATCH_BYTES(n, k) ((int64_t)(n) * (k) * 8)
int isa_copy_paste_u8(const uint8_t* rgb, const uint8_t* sem, const uint8_t* planes, const int32_t* n_objects,
                      const int32_t* xform, const uint32_t* select, int32_t n, int32_t h, int32_t w, int32_t c, int32_t k,
                      int32_t min_area, uint8_t* rgb_out, uint8_t* sem_out, uint8_t* planes_out, int32_t* n_out,
                      int32_t* plan, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- boundary layout converters (the reference passes NCHW fp32: reseg.py:106-110) -----------
 * nchw_to_nhwc: channels [csrc, c) are written as 0; bf16 stores round to nearest even.  Channels at or above c: a dst
 * with ld == rup(c, 8) <= 32, 16-byte aligned src and data and h*w % 4 == 0 is written in whole padded rows (channels
 * [c, ld) become 0); any other dst is written element by element and channels outside [0, c) are left alone.
 * nhwc_to_nchw writes the c channels of src. */
int isa_nchw_to_nhwc(const float* src, int32_t csrc, const isa_tensor* dst, void* stream);
int isa_nhwc_to_nchw(const isa_tensor* src, float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISA_KERNELS_H */
