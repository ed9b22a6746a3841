"""Attention mask-prediction head composed from engine ops.

Reference: reseg.py:78-102,122-126 (stems), attenet2.py:357-407 (DecoderLayer.forward driver),
attenet2.py:443-473 (AttenDecoder), utils.py:457-663 (attention layers), utils.py:816-1112
(UpDecoderLayer / UpAttenLayer / L0Layer), attenet2.py:86-141,204-290 (losses).

What changes vs. the reference's control flow (same results, MI355X-first):
  * nothing leaves the device inside the iteration loop: the reference copies alpha to the CPU,
    samples there and rebuilds Python int lists (attenet2.py:306-332); here argmax / injected samples
    stay in a device int32 vector that the position-code kernel reads;
  * HardAttentionLayer's [B,32,H,W] softmax (utils.py:648-655) is evaluated only for the instance
    each iteration actually selects (B rows, not 32*B);
  * concat order inside the decoder is [gated_up | cross | mask_all | position] so every slice
    starts 16-byte aligned; conv1's weight columns are permuted to match when packed.
"""
import collections
import math
import os

import torch

from . import lib as L
from .engine import Act, Engine, Pro

SKIP_CH = (512, 256, 128, 64, 32)
OUT_CH = (256, 128, 64, 32, 32)
FACTORS = (16, 8, 4, 2, 1)
PYRAMID_W = (16.0, 8.0, 4.0, 2.0, 1.0)     # config.py:51
CE_WEIGHT = 10.0                            # config.py:17
LAMBDA_L, LAMBDA_R = 0.5, 2.0               # config.py:45-46
MAX_ITER = 2                                # config.py:56
DROP_RATE = 0.5                             # config.py:64
ROW_PART = 64 * 4                           # floats of chunk partials per softmax row (ISA_ROW_CHUNKS * 4, isa_kernels.h)
SEG_PART = 64 * 2                           # floats of chunk candidates per row of isa_seg_begin / isa_seg_claim

# One decoder pass: iterations [it0, it0 + G) as G*n images with G BatchNorm statistic groups; the cross branches run on
# stream sc, the level chain on stream sm; defer: its running-statistics updates wait for Engine.flush_bn_running().
Pass = collections.namedtuple("Pass", "it0 G sc sm defer")
# What a pass computes ahead of its levels, one row per (iteration, image): see InstanceHead.front.
Front = collections.namedtuple("Front", "idx alpha s_t targets sums_all")


class InstanceHead:
    def __init__(self, net):
        self.net = net
        self.E: Engine = net.E
        self.drop_rate = DROP_RATE
        # The two flags choose the decoder's pass list (see passes); one driver runs whatever they choose.
        # concurrent HIP streams for the pyramid passes: 1 = none, 2 = odd iterations (the batched pass: its cross chain)
        # on a side stream, 3 = cross chains on the step's stream + one side stream per iteration's level chain
        self.streams = int(os.environ.get("ISA_STREAMS", "2"))
        # all decoder iterations of a train-mode pass as ONE batch of max_iter * B images with a BatchNorm statistic group
        # per iteration (attenet2.py:384-399 runs them one after the other through the same weights): half the launches,
        # twice the work per launch on the low-resolution levels.  0 = one pass per iteration (A/B, bisecting).
        self.batch_iters = os.environ.get("ISA_BATCH_ITERS", "1") != "0"
        self.injected_masks = None       # {(iteration, level, "cross"|"d1"|"d2"): [n, C] keep/(1-p) mask}: parity by injection
        self.sample_in_training = True   # False: greedy point (argmax) also in training; parity tests inject s_t instead
        import ctypes as _C
        self._level_w = (_C.c_float * 5)(*PYRAMID_W)
        self.baseline = None            # device scalar (REINFORCE EMA baseline, attenet2.py:47,266)

    # ------------------------------------------------------------------ stems (reseg.py:78-102)
    def stems(self, x_dec: Act) -> Act:
        E, net = self.E, self.net
        n, h, w = x_dec.n, x_dec.h, x_dec.w
        p1, p2 = "ins_seg_output_1", "ins_seg_output_2"
        y = E.new_act(n, h, w, 32)
        _, s = E.dwconv(x_dec, p1 + ".0.weight", y, bias=p1 + ".0.bias", stats=True)
        y = E.bn(y, s, p1 + ".1", L.ACT_RELU6)
        z = E.new_act(n, h, w, 24)
        _, s = E.conv(y, p1 + ".3.weight", z, bias=p1 + ".3.bias", stats=True)
        e1 = E.new_act(n, h, w, 24)
        E.bn_out(z, s, p1 + ".4", L.ACT_RELU6, e1)
        y = E.new_act(n, h, w, 48)
        _, s = E.conv(e1, p2 + ".0.weight", y, bias=p2 + ".0.bias", stats=True)
        y = E.bn(y, s, p2 + ".1", L.ACT_RELU6)
        z = E.new_act(n, h, w, 48)
        _, s = E.dwconv(y, p2 + ".3.weight", z, bias=p2 + ".3.bias", stats=True)
        z = E.bn(z, s, p2 + ".4", L.ACT_RELU6)
        y = E.new_act(n, h, w, 24)
        _, s = E.conv(z, p2 + ".6.weight", y, bias=p2 + ".6.bias", stats=True)
        x_enc = E.new_act(n, h, w, 24)
        return E.bn_out(y, s, p2 + ".7", L.ACT_NONE, x_enc, res=e1)

    # ------------------------------------------------------------------ a7 SpatialAttentionLayer
    def spatial_attention(self, x: Act, sem: torch.Tensor) -> Act:
        E, P = self.E, self.E.params
        n, c, Lp = x.n, x.c, x.h * x.w
        pre = "decoder.s_sp"
        dot, chansum = E.scratch(n * Lp), E.scratch(n * c)
        E.lib.isa_mask_dot(x.d(), sem, P.ptr(pre + ".l_v.weight"), P.ptr(pre + ".l_v.bias"), dot, chansum, E.st())
        beta, rowstat = E.f32(n * Lp), E.f32(n * 4)
        E.lib.isa_sp_softmax(dot, sem, chansum, P.ptr(pre + ".l_h.weight"), P.ptr(pre + ".spatial_fc.1.weight"),
                             P.ptr(pre + ".spatial_fc.1.bias"), n, c, Lp, beta, rowstat, E.f32(n * ROW_PART), E.st())
        scale, shift, mean, invstd = (E.f32(c) for _ in range(4))
        stats = E.scratch(2 * c * 8)
        if E.bn_train:
            E.lib.isa_scaled_stats(x.d(), beta, stats, E.st())
            P.int_buffers[pre + ".bn.num_batches_tracked"] += 1
        E.bn_finalize(stats if E.bn_train else None, float(n * Lp), pre + ".bn", E.running_ptrs(pre + ".bn"), scale, shift,
                      mean, invstd, c, 1, 1)
        out = E.new_act(n, x.h, x.w, c)
        E.lib.isa_sp_apply(x.d(), beta, sem, scale, shift, out.d(), E.st())
        if E.record:
            train = 1 if E.bn_train else 0

            def bwd():
                scr = E.scratch(3 * c + 2 * ((n + 3) // 4 * 4) + 2 * n * Lp)
                acc = E.grads.claim(x, E)
                E.lib.isa_sp_bwd(E.grads.grad_of(out).d(), x.d(), beta, sem, dot, rowstat, chansum, scale, mean, invstd,
                                 P.ptr(pre + ".l_v.weight"), P.ptr(pre + ".l_h.weight"),
                                 P.ptr(pre + ".spatial_fc.1.weight"), float(n * Lp), train, scr, E.grads.grad_of(x).d(),
                                 acc, P.gptr(pre + ".bn.weight"), P.gptr(pre + ".bn.bias"), P.gptr(pre + ".l_v.weight"),
                                 P.gptr(pre + ".l_v.bias"), P.gptr(pre + ".l_h.weight"),
                                 P.gptr(pre + ".spatial_fc.1.weight"), P.gptr(pre + ".spatial_fc.1.bias"), E.st())
            E.tape.append(bwd)
        return out

    # ------------------------------------------------------------------ a8/a9 HardAttentionLayer front
    def hard_attention_scores(self, s: Act, sem: torch.Tensor) -> torch.Tensor:
        """Returns pro_merge as an fp32 [n, h*w] map."""
        E, P = self.E, self.E.params
        n, h, w = s.n, s.h, s.w
        pre = "decoder.attend"
        sp = E.new_act(n, h, w, s.c)
        E.lib.isa_avgpool3(s.d(), None, sp.d(), 0, E.st())
        if E.record:
            def bwd_pool():      # 3x3 mean with zero padding is self-adjoint
                acc = E.grads.claim(s, E)
                E.lib.isa_avgpool3(E.grads.grad_of(sp).d(), None, E.grads.grad_of(s).d(), acc, E.st())
            E.tape.append(bwd_pool)
        e1 = E.new_act(n, h, w, 12)
        E.conv(sp, pre + ".l1.weight", e1, bias=pre + ".l1.bias")
        e2 = E.new_act(n, h, w, 1)
        e1t = E.act_out(e1, L.ACT_TANH, E.new_act(n, h, w, 12))        # tanh once, not once per tap
        E.conv(e1t, pre + ".attend_fc.1.weight", e2, taps=9, bias=pre + ".attend_fc.1.bias")
        am, v, mean_var = E.f32(2 * n), E.f32(n), E.f32(2)
        train = 1 if E.bn_train else 0
        rm, rv = P.ptr(pre + ".bn.running_mean"), P.ptr(pre + ".bn.running_var")
        if train:
            E.lib.isa_maskbn_stats(e2.d(), sem, None, am, E.st())
        E.lib.isa_maskbn_finalize(am, v, n, 0, mean_var, rm, rv, E.BN_MOMENTUM, train, E.st())
        if train:
            E.lib.isa_maskbn_stats(e2.d(), sem, mean_var, v, E.st())
            E.lib.isa_maskbn_finalize(am, v, n, 1, mean_var, rm, rv, E.BN_MOMENTUM, 1, E.st())
            P.int_buffers[pre + ".bn.num_batches_tracked"] += 1
        merge = E.f32(n * h * w)
        E.lib.isa_maskbn_apply_pool(e2.d(), sem, mean_var, P.ptr(pre + ".bn.weight"), P.ptr(pre + ".bn.bias"), E.BN_EPS,
                                    merge, E.st())
        self.dmerge = None
        if E.record:
            dmerge = E.scratch(n * h * w)       # zero at step start; filled by the per-iteration closures
            self.dmerge = dmerge

            def bwd_bn():
                red4, k2 = E.scratch(4), E.f32(2)
                acc = E.grads.claim(e2, E)
                E.lib.isa_maskbn_bwd(e2.d(), sem, dmerge, mean_var, P.ptr(pre + ".bn.weight"), E.BN_EPS, am, train, red4,
                                     k2, P.gptr(pre + ".bn.weight"), P.gptr(pre + ".bn.bias"), E.grads.grad_of(e2).d(), acc,
                                     E.st())
            E.tape.append(bwd_bn)
        return merge

    # ------------------------------------------------------------------ pyramid decoder
    def passes(self, max_iter):
        """The decoder passes of a step that runs max_iter iterations.  The iterations share weights and backbone
        features but not data (attenet2.py:384-399 runs them one after the other), and inside an iteration the cross
        branch of every level only reads the backbone.  Most of these launches are too small to fill 256 CUs (16x16 ...
        64x64 maps), so independent chains run on separate HIP streams.
        Train-mode BatchNorm, 2..4 iterations (batch_iters): ONE pass over max_iter * n images, rows ordered
        [iteration][image].  BatchNorm statistics stay per iteration (isa_tensor.groups = G), running statistics take the
        G updates in iteration order inside isa_bn_finalize, the REINFORCE baseline EMA runs in iteration order inside
        isa_head_loss.  The cross chain runs beside the level chain on side stream 1 (streams >= 2), one edge per level.
        Otherwise one pass per iteration.  streams == 2 (default): odd iterations run whole on side stream 1, one fork
        and one join per pass (34.3 -> 30.0 ms/step at the BASELINE shape under hipGraph replay).  streams == 3: the
        cross chains of all iterations stay on the step's own stream, the level chain of iteration i runs on side stream
        1 + i % 2, one edge per level; measured slower (31.9 ms: every extra cross-stream edge costs more than the finer
        overlap returns; cross chains on their own side streams 32.4 - 33.9 ms).  Every edge has the origin stream at
        one end: hipGraph capture of side -> side edges crashes inside ROCm 7.2's hipStreamEndCapture
        (scripts/graph_probe.py).
        What the sequential order guaranteed is restored explicitly: a BatchNorm layer must see iteration 0's update
        first, so only iteration 0's in-launch update is kept when iterations can overlap and later ones are queued
        (Pass.defer) for flush_bn_running() after the join, in iteration order (isa_bn_running_update); gradients of
        backbone features read from a side stream are accumulated per stream and merged (GradBook.merge_shared); loss
        assembly stays on the origin stream."""
        if self.batch_iters and self.E.bn_train and 2 <= max_iter <= 4:
            return [Pass(0, max_iter, 1 if self.streams >= 2 else 0, 0, False)]
        ns = self.streams if max_iter >= 2 else 1
        assert ns in (1, 2, 3), "ISA_STREAMS must be 1, 2 or 3"
        sc_sm = {1: lambda it: (0, 0), 2: lambda it: (it % 2, it % 2), 3: lambda it: (0, 1 + it % 2)}[ns]
        return [Pass(it, 1, *sc_sm(it), self.E.bn_train and it >= 1 and ns > 1) for it in range(max_iter)]

    def fg_pyramid(self, sem_map, nobj, n, H, W):
        """mask_all: the foreground map at the five pyramid sizes (sem_map itself at full size)."""
        E = self.E
        out = []
        for f in FACTORS[:-1]:
            m = E.f32(n * (H // f) * (W // f))
            E.lib.isa_pool_target(None, None, sem_map, nobj, n, H, W, f, m, n, E.st())
            out.append(m)
        return out + [sem_map]

    def front(self, p, merge, ins, idx_dev, injected_s_t, training, n, H, W):
        """What a pass needs before its first level, for its G*n rows: instance softmax, glimpse point, the five pyramid
        targets, and the zeroed sums isa_head_loss reads ([level][iteration][image][8])."""
        E = self.E
        Lp, R, nobj = H * W, p.G * n, ins.shape[1]
        idx = idx_dev[p.it0:p.it0 + p.G].reshape(-1).contiguous()          # [G*n] instance order
        alpha, rowstat = E.f32(R * Lp), E.f32(2 * R)
        E.lib.isa_ins_softmax(merge, ins, idx, R, nobj, Lp, alpha, rowstat, n, E.f32(R * ROW_PART), E.st())
        if injected_s_t is None:
            # attenet2.py:304-321 `sample`: training draws s_t ~ Multinomial(alpha), eval takes the argmax.
            # The draw is argmax(alpha / Exp(1)) (the exponential-race form torch.multinomial itself uses
            # for one sample); torch supplies the random numbers (graph-safe generator), the row argmax is ours.
            race = None
            if training and self.sample_in_training:
                race = torch.empty(R, Lp, dtype=torch.float32, device=alpha.device).exponential_(1.0)
            s_t = E.arena.alloc((R,), torch.int32)
            E.lib.isa_row_argmax(alpha, race, R, Lp, s_t, E.st())
        elif p.G == 1:
            s_t = injected_s_t[p.it0]
        else:
            s_t = E.arena.alloc((R,), torch.int32)
            for g in range(p.G):
                s_t[g * n:(g + 1) * n].copy_(injected_s_t[p.it0 + g])
        targets = []
        for f in FACTORS:
            t = E.f32(R * (H // f) * (W // f))
            E.lib.isa_pool_target(ins, idx, None, nobj, R, H, W, f, t, n, E.st())
            targets.append(t)
        return Front(idx, alpha, s_t, targets, E.scratch(5 * 8 * R))

    def drop_masks(self, passes, n, training):
        """All Dropout2d masks of a step (utils.py:869-892: three per level and iteration) from ONE torch.rand draw and one
        launch - per-mask draws were ~120 five-microsecond launches per step.  Returns [pass][level] {cross, d1, d2} of
        [G*n, C] arrays ([iteration][image] rows), taken from the draw in the order pass, level, kind.  Only the active
        kinds are drawn (cross: train-mode BatchNorm, the module's own nn.Dropout2d; d1 / d2: training); an inactive mask
        is absent, but a pass with G > 1 gets all ones for cross: its broadcast materialising pass always takes a
        per-image scale.  injected_masks replaces the draw."""
        E, inj = self.E, self.injected_masks
        kinds = [k for k, on in (("cross", E.bn_train), ("d1", training), ("d2", training)) if on and self.drop_rate > 0]
        total = sum(len(kinds) * p.G * n * oc for p in passes for oc in OUT_CH)
        pool, cur = None, 0
        if inj is None and total:
            u = torch.rand(total, device=E.device)           # torch supplies the random numbers (graph-safe generator)
            pool = torch.empty_like(u)
            E.lib.isa_dropout_mask(u, total, 1.0 - self.drop_rate, pool, E.st())
        out = []
        for p in passes:
            R = p.G * n
            out.append([])
            for lvl, oc in enumerate(OUT_CH):
                masks = {}
                for kind in kinds:
                    if inj is not None:
                        masks[kind] = torch.cat([inj[p.it0 + g, lvl, kind].to(E.device, torch.float32).reshape(n, oc)
                                                 for g in range(p.G)])
                    else:
                        masks[kind] = pool[cur:cur + R * oc].view(R, oc)
                        cur += R * oc
                if p.G > 1 and "cross" not in masks:
                    ones = getattr(self, "_ones", None)
                    if ones is None or ones.numel() < R * oc:
                        ones = self._ones = torch.ones(R * max(OUT_CH), device=E.device)
                    masks["cross"] = ones[:R * oc].view(R, oc)
                out[-1].append(masks)
        return out

    def level_cross(self, lvl, skip: Act, masks, G=1):
        """The `cross` branch of one UpAttenLayer (utils.py:1058-1075): IR -> Dropout2d(module) -> IR on the backbone
        feature.  It does not depend on the previous level, so it runs on its own stream next to the level chain.
        Returns the concat buffer (its cross slice written).
        G > 1 (all decoder iterations in one pass): the first block sees the same input and weights in every
        iteration, so it is evaluated ONCE (E.repeated(G): running statistics advance G times) and only its Dropout2d
        differs - the materialising pass writes G masked copies (masks["cross"] is [G*n, C])."""
        E, net = self.E, self.net
        ua = "decoder.bone.upAtten%d.UpAtten" % lvl
        n, h, w = skip.n, skip.h, skip.w
        out_ch, f = OUT_CH[lvl], FACTORS[lvl]
        nb = int(math.log2(f))
        naux = 2 * nb + 2
        ccross = out_ch - naux
        width = out_ch if lvl == 0 else 2 * out_ch
        cat = E.new_act(G * n, h, w, width, ld=width, groups=G)
        cross_off = 0 if lvl == 0 else out_ch
        mid = E.new_act(G * n, h, w, out_ch, groups=G)
        if G > 1:
            with E.repeated(G):
                net.block_ir(skip, ua + ".cross.up_feature.0", mid, oscale=masks["cross"])
        else:
            net.block_ir(skip, ua + ".cross.up_feature.0", mid, oscale=masks.get("cross"))
        net.block_ir(mid, ua + ".cross.up_feature.2", cat.slice(cross_off, ccross))
        return cat

    def level_main(self, lvl, cat: Act, x_prev: Act, pred_prev: Act, mask_all, s_t, W_full, training, masks):
        """The rest of one UpDecoderLayer (utils.py:869-892) once the cross slice of `cat` is there.  Returns (x, pred).
        With cat.groups > 1 the batch holds all decoder iterations ([iteration][image]); mask_all is the one map per
        image they share, s_t and the masks are per (iteration, image)."""
        E, net = self.E, self.net
        pre = "decoder.bone.upAtten%d" % lvl
        ua = pre + ".UpAtten"
        n, h, w = cat.n, cat.h, cat.w
        out_ch, f = OUT_CH[lvl], FACTORS[lvl]
        nb = int(math.log2(f))
        naux = 2 * nb + 2
        ccross = out_ch - naux
        cross_off = 0 if lvl == 0 else out_ch
        up = None
        if lvl > 0:
            up = E.like(cat, out_ch)
            E.conv(x_prev, ua + ".up.weight", up, bias=ua + ".up.bias", transposed=True)
            gated = cat.slice(0, out_ch)
            gmap = E.f32(n * h * w) if E.record else None
            E.lib.isa_gate(up.d(), pred_prev.d(), gated.d(), gmap, E.st())
            if E.record:
                def bwd_gate(up=up, pred_prev=pred_prev, gated=gated, gmap=gmap):
                    du = E.scratch(n * h * w)
                    acc_up = E.grads.claim(up, E)
                    acc_pred = E.grads.claim(pred_prev, E)
                    E.lib.isa_gate_bwd(E.grads.grad_of(gated).d(), up.d(), gmap, E.grads.grad_of(up).d(), acc_up, du,
                                       E.grads.grad_of(pred_prev).d(), acc_pred, E.st())
                E.tape.append(bwd_gate)
        aux = cat.slice(cross_off + ccross, naux)
        E.lib.isa_concat_aux(aux.d(), mask_all, s_t, W_full, f, nb, n // cat.groups, E.st())
        if lvl == 0:
            kmap = None
        else:   # physical [gated(out) | cross(ccross) | aux] -> source [cross | gated | aux]
            kmap = [ccross + k for k in range(out_ch)] + list(range(ccross)) + \
                   [ccross + out_ch + k for k in range(naux)]
        y = E.like(cat, out_ch)
        _, s = E.conv(cat, ua + ".conv1.0.weight", y, stats=True, kmap=kmap)
        x = E.like(cat, out_ch)
        E.bn_out(y, s, ua + ".conv1.1", L.ACT_RELU, x, bscale=masks.get("d1"))
        x2 = E.like(cat, out_ch)
        net.block_ir(x, ua + ".dilation_part1.0", x2)
        x3 = E.like(cat, out_ch)
        self._block_ir_ext(x2, ua + ".dilation_part1.1", x3, res2=up, oscale=masks.get("d2"))
        x4 = E.like(cat, out_ch)
        net.block_ir(x3, ua + ".dilation_part2.0", x4)
        x5 = E.like(cat, out_ch)
        net.block_ir(x4, ua + ".dilation_part2.1", x5)
        # L0Layer (utils.py:696-774): conv3x3 -> LeakyReLU -> conv3x3
        hmid = E.like(cat, out_ch // 2)
        E.conv(x5, pre + ".pred.l_i.weight", hmid, taps=9, bias=pre + ".pred.l_i.bias")
        pred = E.like(cat, 2)
        hact = E.act_out(hmid, L.ACT_LEAKY, E.like(cat, out_ch // 2))     # once, not once per tap
        E.conv(hact, pre + ".pred.last_fc.1.weight", pred, taps=9, bias=pre + ".pred.last_fc.1.bias")
        return x5, pred

    def _block_ir_ext(self, x, pre, out, res2=None, oscale=None):
        """InvertedResidual whose materialising pass also adds `res2` and applies a Dropout2d mask
        to the sum (utils.py:1104-1110: x = dilation_part1(x); x = x + x1; x = dropout2d(x))."""
        E = self.E
        chid = E.params.shapes[pre + ".conv.0.weight"][0]
        cout = E.params.shapes[pre + ".conv.6.weight"][0]
        y1 = E.like(x, chid)
        _, s1 = E.conv(x, pre + ".conv.0.weight", y1, stats=True)
        y1 = E.bn(y1, s1, pre + ".conv.1", L.ACT_RELU6)
        y2 = E.like(x, chid)
        _, s2 = E.dwconv(y1, pre + ".conv.3.weight", y2, stats=True)
        y2 = E.bn(y2, s2, pre + ".conv.4", L.ACT_RELU6)
        y3 = E.like(x, cout)
        _, s3 = E.conv(y2, pre + ".conv.6.weight", y3, stats=True)
        return E.bn_out(y3, s3, pre + ".conv.7", L.ACT_NONE, out, res=x if x.c == cout else None,
                        res2=res2, oscale=oscale)

    # ------------------------------------------------------------------ discriminative loss on the embedding
    def disc_loss(self, x_enc: Act, ins: torch.Tensor, n_obj: torch.Tensor) -> torch.Tensor:
        """The discriminative embedding loss (LabelOps.disc_loss in the step's arena; settings in net.disc) on the instance
        embedding x_enc against the step's instance planes: the label map once, the four forward launches, and one tape
        closure that adds the loss's gradient into d(x_enc).  Returns scal [8]."""
        E, net = self.E, self.net
        n, k = ins.shape[0], ins.shape[1]
        assert ins.dtype == torch.int64 and 1 <= k <= L.DISC_MAX_K, "instance planes: int64 [n,K,h,w], K <= 32"
        labels, _ = net.maps.labels_from_planes(ins, "instance planes")
        assert labels.numel() == n * x_enc.h * x_enc.w, "instance planes do not match the embedding"
        scal, _, grad = net.maps.disc_loss(x_enc, labels.view(n, -1), k, n_obj, net.disc.cfg, net.disc.norm)
        if E.record:
            def bwd_disc():
                acc = E.grads.claim(x_enc, E)
                grad(E.grads.grad_of(x_enc), acc)
            E.tape.append(bwd_disc)
        return scal

    # ------------------------------------------------------------------ driver (attenet2.py:357-407)
    def forward(self, x_dec: Act, feats, sem_map: torch.Tensor, ins: torch.Tensor, n_ins, training: bool,
                selected_idx, injected_s_t=None, capture=None, idx_dev=None, disc=None):
        """sem_map: fp32 [n, h*w] {0,1}; ins: int64 [n,32,h,w] on device; n_ins: host ints;
        selected_idx[b]: instance order; injected_s_t: optional list of int32 device vectors (train
        sampling is injected, SURVEY §7 'RNG parity').  disc (the trainer's, when the discriminative embedding loss is on):
        dict(n_obj = the object counts, int32 [n] on the device); it receives `scal`, the loss's eight scalars.
        Returns dict of per-iteration records."""
        E = self.E
        n, H, W = x_dec.n, x_dec.h, x_dec.w
        Lp = H * W
        nobj = ins.shape[1]
        x_enc = self.stems(x_dec)
        if disc is not None:
            disc["scal"] = self.disc_loss(x_enc, ins, disc["n_obj"])
        s = self.spatial_attention(x_enc, sem_map)
        merge = self.hard_attention_scores(s, sem_map)
        nmin = int(min(int(v) for v in n_ins))
        max_iter = min(MAX_ITER, nmin) if training else nmin
        mask_all = self.fg_pyramid(sem_map, nobj, n, H, W)
        if idx_dev is None:          # [max_iter, n] int32 instance order; pre-staged by the graph-captured step
            idx_dev = self.order_tensor(selected_idx, max_iter, n).to(E.device)
        skips = [feats[4], feats[3], feats[2], feats[1], feats[0]]
        iters = []
        scal = E.scratch(4)          # {ins_cost (finite part), criterion, ins_ce_loss, ins_dice_loss}
        if self.baseline is None:
            self.baseline = torch.zeros(1, dtype=torch.float32, device=E.device)
        if capture is not None:
            capture.update(x_enc=x_enc, s_sp=s, merge=merge)
        # One driver for every configuration: the pass list is the only thing the mode decides (one batched pass, or one
        # pass of G = 1 per iteration).  Fronts and masks on the step's stream, forks, the five levels, joins, losses.
        passes = self.passes(max_iter)
        fronts = [self.front(p, merge, ins, idx_dev, injected_s_t, training, n, H, W) for p in passes]
        masks = self.drop_masks(passes, n, training)
        side = sorted({sid for p in passes for sid in (p.sc, p.sm) if sid})
        if side:
            for sk in skips:
                E.grads.share(sk)
            if E.record:
                E.tape.append(lambda: E.grads.merge_shared(E))      # runs after the reversed forks have joined stream 0
        for sid in side:                    # all forks up front: a fork issued later would wait for iteration 0's chain
            E.sync(0, sid)
        chain = [(None, None)] * len(passes)                        # (x, pred) of each pass's previous level
        preds = [[] for _ in passes]
        for lvl in range(5):                # level-major issue order: the cross chains of all passes interleave
            for k, (p, fr) in enumerate(zip(passes, fronts)):
                R = p.G * n
                E.defer_bn_running = p.defer
                with E.on(p.sc):
                    cat = self.level_cross(lvl, skips[lvl], masks[k][lvl], p.G)
                E.sync(p.sc, p.sm)
                with E.on(p.sm):
                    x, pred = self.level_main(lvl, cat, *chain[k], mask_all[lvl], fr.s_t, W, training, masks[k][lvl])
                    E.lib.isa_mask_loss_sums(pred.d(), fr.targets[lvl], None, fr.sums_all[lvl * 8 * R:(lvl + 1) * 8 * R],
                                             E.st())
                chain[k] = (x, pred)
                preds[k].append(pred)
                if capture is not None:
                    for g in range(p.G):
                        capture["it%d.L%d.x" % (p.it0 + g, lvl)] = x.images(g * n, n)
                        capture["it%d.L%d.pred" % (p.it0 + g, lvl)] = pred.images(g * n, n)
        E.defer_bn_running = False
        for sid in sorted({p.sm for p in passes if p.sm}):          # a cross-only side stream was joined level by level
            E.sync(sid, 0)
        E.flush_bn_running()
        hw = [(H // f) * (W // f) for f in FACTORS]
        for k, (p, fr) in enumerate(zip(passes, fronts)):           # losses in iteration order: the baseline is an EMA
            R = p.G * n
            coef, adv = E.f32(5 * 4 * R), E.f32(R)
            E.lib.isa_head_loss(fr.sums_all, fr.alpha, fr.s_t, Lp, n, self._level_w, CE_WEIGHT, LAMBDA_L, LAMBDA_R,
                                1.0 / max_iter, self.baseline, 1 if training else 0, coef, adv, scal, p.G, E.st())
            if E.record:
                def bwd_losses(fr=fr, R=R, preds=preds[k], coef=coef, adv=adv):
                    for lvl in range(5):
                        acc = E.grads.claim(preds[lvl], E)
                        E.lib.isa_mask_loss_grad(preds[lvl].d(), fr.targets[lvl], None, coef[lvl * 4 * R:(lvl + 1) * 4 * R],
                                                 E.grads.grad_of(preds[lvl]).d(), acc, E.st())
                    E.lib.isa_ins_softmax_bwd(fr.alpha, ins, fr.idx, fr.s_t, adv, R, nobj, Lp, self.dmerge, n, E.st())
                E.tape.append(bwd_losses)
            for g in range(p.G):                                    # per-iteration views of the pass's tensors
                rows = lambda t, per: t[g * n * per:(g + 1) * n * per]
                iters.append(dict(idx=rows(fr.idx, 1), alpha=rows(fr.alpha, Lp), s_t=rows(fr.s_t, 1),
                                  targets=[rows(fr.targets[l], hw[l]) for l in range(5)],
                                  preds=[q.images(g * n, n) for q in preds[k]],
                                  sums=[rows(fr.sums_all[l * 8 * R:(l + 1) * 8 * R], 8) for l in range(5)]))
        return dict(iters=iters, max_iter=max_iter, merge=merge, x_enc=x_enc, scal=scal)

    # ------------------------------------------------------------------ ground-truth-free inference (ReSeg.segment)
    def segment(self, x_dec: Act, feats, sem_map: torch.Tensor, max_objects: int, injected_s_t=None, capture=None):
        """One glimpse point per object, one decoder pass per point, without ground truth: the point of an iteration is
        the first arg-max of `merge` over the foreground no instance has claimed yet (the arg-max the ground-truth path
        takes over an instance plane, isa_ins_softmax + isa_row_argmax, without the softmax: it does not move an
        arg-max); the instance claims the remaining pixels its level-4 prediction calls foreground, and the point.
        sem_map: fp32 {0,1} [n, h*w].  Returns (labels uint8 [n,h,w], count int32 [n]) in the step's arena.
        Eval mode only, so the cross branches (backbone features only) run ONCE and their five concat buffers are kept;
        an iteration rewrites the gated and aux slices (level_main), on buffers the iterations share (the arena cursor
        is rewound): 20 of the 30 InvertedResidual blocks of a pass, and memory that does not grow with max_objects.
        Per iteration: the level chain, isa_seg_claim (two launches: labels + next point, then the fold) and at most
        one 4-byte device-to-host read, taken one iteration late so that the host never waits for the pass it has just
        queued - a pass in which no image is active changes nothing."""
        E = self.E
        assert not E.bn_train and not E.record, "segment() runs in eval mode, without a tape"
        n, H, W = x_dec.n, x_dec.h, x_dec.w
        Lp = H * W
        assert 1 <= max_objects <= 255, "labels are uint8: max_objects must be in 1..255"
        x_enc = self.stems(x_dec)
        s = self.spatial_attention(x_enc, sem_map)
        merge = self.hard_attention_scores(s, sem_map)
        mask_all = self.fg_pyramid(sem_map, 1, n, H, W)
        if capture is not None:
            capture.update(x_enc=x_enc, s_sp=s, merge=merge)
        skips = [feats[4], feats[3], feats[2], feats[1], feats[0]]
        cats = [self.level_cross(lvl, skips[lvl], {}) for lvl in range(5)]
        labels = E.arena.alloc((n, H, W), torch.uint8)
        ints = E.arena.alloc((3 * n + 4,), torch.int32)          # count | active | s_t | the "any image active" word
        count, active, s_t, any_dev = ints[:n], ints[n:2 * n], ints[2 * n:3 * n], ints[3 * n:3 * n + 1]
        part = E.f32(n * SEG_PART)
        E.lib.isa_seg_begin(sem_map, merge, n, Lp, labels, count, s_t, active, any_dev, part, E.st())
        iters = max_objects if injected_s_t is None else len(injected_s_t)
        assert iters <= 255
        flags = self._seg_flags(iters + 1) if injected_s_t is None else None
        if flags is not None:
            self._seg_flag_read(flags, 0, any_dev)               # flag t: "iteration t has an active image"
        mark, smark = E.arena.cursor, E.arena.stats_cursor
        done = 0
        for t in range(iters):
            if flags is not None and t >= 1 and not self._seg_flag_wait(flags, t - 1):
                break                                            # iteration t-1 had nothing to do, so neither has t
            E.arena.cursor, E.arena.stats_cursor = mark, smark   # the iterations share their buffers
            pt = s_t if injected_s_t is None else injected_s_t[t]
            x = pred = None
            for lvl in range(5):
                x, pred = self.level_main(lvl, cats[lvl], x, pred, mask_all[lvl], pt, W, False, {})
                if capture is not None:                          # copies: the next iteration reuses the buffers
                    capture["it%d.L%d.pred" % (t, lvl)] = Act(pred.buf.clone(), pred.c0, pred.c)
            if capture is not None:
                capture["it%d.s_t" % t] = pt.clone()
            E.lib.isa_seg_claim(pred.d(), sem_map, merge, pt, labels, count, active, s_t, any_dev, part, E.st())
            if flags is not None:
                self._seg_flag_read(flags, t + 1, any_dev)
            done = t + 1
        self.seg_passes = done                                   # decoder passes issued (tests, bench_segment)
        return labels, count

    def _seg_flags(self, k):
        """Pinned host words for the stop test and one event per word (reused from call to call)."""
        st = getattr(self, "_seg_flag_state", None)
        if st is None or st[0].numel() < k:
            st = self._seg_flag_state = (torch.zeros(256, dtype=torch.int32).pin_memory(),
                                         [torch.cuda.Event() for _ in range(256)])
        return st

    def _seg_flag_read(self, flags, i, any_dev):
        flags[0][i:i + 1].copy_(any_dev, non_blocking=True)
        flags[1][i].record(torch.cuda.current_stream())

    def _seg_flag_wait(self, flags, i):
        flags[1][i].synchronize()
        return int(flags[0][i]) != 0

    @staticmethod
    def order_tensor(selected_idx, max_iter, n):
        return torch.tensor([[selected_idx[b][it] for b in range(n)] for it in range(max_iter)],
                            dtype=torch.int32).reshape(max_iter, n)

    # ------------------------------------------------------------------ host-side scalar assembly
    @staticmethod
    def scalars_from_sums(rec, training, baseline=0.0):
        """Reference outputs (ins_cost, criterion, ins_ce_loss, ins_dice_loss) from the per-level
        per-image sums.  Host arithmetic on 5*B*7 floats (validation / logging path; the training
        path assembles the same quantities on device in isa_head_loss)."""
        tot = dict(loss=0.0, criterion=0.0, ce=0.0, dice=0.0)
        nan = False
        max_iter = rec["max_iter"]
        for itrec in rec["iters"]:
            S = [s.view(-1, 8).double().cpu() for s in itrec["sums"]]
            last = S[-1]
            nimg = last.shape[0]
            cnt = last[:, 6]
            eval_ce = float(last[:, 4].sum() / cnt.sum())
            dice1 = 1.0 - (2 * last[:, 0] + 1.0) / (last[:, 1] + last[:, 2] + 1.0)
            if not training:
                dice2 = 1.0 - (2 * last[:, 0] + 1.0) / (last[:, 5] + last[:, 2] + 1.0)
                tot["loss"] = tot["loss"] + dice2
                tot["criterion"] = tot["criterion"] + (eval_ce + dice1)
            else:
                nan = True
                tot["criterion"] = tot["criterion"] + (eval_ce + float(dice1.sum()))
            tot["ce"] += eval_ce
            tot["dice"] += float(dice1.mean())
        out = dict(ins_ce_loss=tot["ce"] / max_iter, ins_dice_loss=tot["dice"] / max_iter)
        if training:
            out["ins_cost"] = float("nan")
            out["criterion"] = float(tot["criterion"]) / max_iter
        else:
            out["ins_cost"] = float((tot["loss"] / max_iter).mean())
            out["criterion"] = float((tot["criterion"] / max_iter).mean())
        return out
