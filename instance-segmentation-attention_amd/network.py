"""The ReSeg hot path composed from engine ops (reference: code/lib/archs/reseg.py:106-130).

Buffer plan (NHWC, one buffer per pyramid level, zero-copy concats — see DESIGN.md §layout):
  L256 buf[.,64]  = [ x1 (inc out, 32) | up4 convT out (32) ]      -> up4 reads the whole row
  L128 buf[.,128] = [ conv(32) | mean2x2(32) | up3 convT (64) ]    x2 = first 64
  L64  buf[.,256] = [ conv(64) | mean(64)   | up2 convT (128) ]    x3 = first 128
  L32  buf[.,512] = [ conv(128)| mean(128)  | up1 convT (256) ]    x4 = first 256
  L16  buf[.,512] = [ conv(256)| mean(256) ]                       x5
so torch.cat in unet_parts.py:60,91 costs nothing: producers write into channel slices.
"""
import torch

from . import lib as L
from .engine import Act, Engine, Pro, rup
from .labelmaps import DISC_FORMS, DiscCriterion, LabelOps  # noqa: F401  (the names are imported from here too)


CRITERIA = ("CE", "Dice", "Multi", "Lovasz", "CELovasz")
LOVASZ_SCRATCH_BYTES = 256 << 20     # above this the Lovasz criterion sorts its classes in groups


def lovasz_class_group(K, pixels, backward):
    """Classes the Lovasz criterion sorts at once: all K, or as many as keep its scratch under LOVASZ_SCRATCH_BYTES.  Per
    element of a group: keys and values, in, out and temporary (24 bytes), and at most 0.63 byte of histogram table, tile
    counts and loss partials (1284 bytes a tile of 2048); per element of all K classes: the 4-byte gradient coefficient
    when there is a backward.  G, scale and the segment losses (16 bytes a segment) are not counted.
    Never less than 1: where one class alone, or the gradient coefficients alone, exceed the budget (K * pixels above
    64 M with a backward, pixels above 10 M without), the criterion still runs, one class at a time, and takes what that
    needs: 25 bytes a pixel on top of the coefficients."""
    fixed = 4 * K * pixels if backward else 0
    return max(1, min(K, (LOVASZ_SCRATCH_BYTES - fixed) // (25 * pixels)))


class SemCriterion:
    """The trainer's semantic criterion (Model.__define_criterion, model.py:102-133): criterion type, class weights,
    optimize_bg.  Its settings live in ONE device buffer allocated here, once, and rewritten in place: a captured
    hipGraph reads them at replay time.  Layout (include/isa_kernels.h, isa_sem_loss_k_*): {use_ce, use_dice,
    optimize_bg, lovasz_only_present, w_0 .. w_{K-1}}; no weights = all ones (the same CE and Dice as unweighted).
    "Lovasz" / "CELovasz": the Lovasz-Softmax loss (lovasz_losses.py:156-196), alone or added to CE; class weights are
    the CE term's.  lovasz_per_image sets the segment geometry, so it belongs to a captured step's configuration.
    `legacy`: the shipped combination (K = 2, Multi, no weights, fg only) runs the 2-class kernels it always ran.
    The border term (set_border) weighs the CE of every pixel by the U-Net border map of the step's
    instance targets: its {w0, sigma} live in a second device buffer, `border`, rewritten in place; on / off belongs to a
    captured step's configuration (border_key()), the values do not.  With it on no combination is `legacy`."""

    def __init__(self, n_classes, device):
        self.K = n_classes
        self.cfg = torch.zeros(4 + n_classes, dtype=torch.float32, device=device)
        self.border = torch.tensor([0.0, 5.0], dtype=torch.float32, device=device)
        self.border_on, self.border_weight, self.border_sigma = False, 0.0, 5.0
        self.set("Multi", None, False)

    def set(self, criterion="Multi", class_weights=None, optimize_bg=False, lovasz_per_image=False,
            lovasz_only_present=False):
        assert criterion in CRITERIA, "criterion must be one of %s" % (CRITERIA,)
        K = self.K
        if criterion == "Lovasz" and class_weights is not None:
            raise ValueError("class_weights weigh the CE term: the Lovasz criterion has none (use CELovasz)")
        if criterion == "Lovasz" and self.border_on:
            raise ValueError("the border weight weighs the CE term: the Lovasz criterion has none (use CELovasz)")
        if class_weights is not None:
            class_weights = [float(v) for v in class_weights]
            if len(class_weights) != K:
                raise ValueError("class_weights: %d values for %d classes" % (len(class_weights), K))
            if min(class_weights) < 0 or sum(class_weights[0 if optimize_bg else 1:]) <= 0:
                raise ValueError("class_weights must be non-negative with a positive sum over the optimised classes")
        self.criterion, self.class_weights, self.optimize_bg = criterion, class_weights, bool(optimize_bg)
        self.ce, self.dice = criterion in ("CE", "Multi", "CELovasz"), criterion in ("Dice", "Multi")
        self.lovasz = criterion in ("Lovasz", "CELovasz")
        self.lovasz_per_image, self.lovasz_only_present = bool(lovasz_per_image), bool(lovasz_only_present)
        self._set_legacy()
        w = class_weights if class_weights is not None else [1.0] * K
        self.cfg.copy_(torch.tensor([float(self.ce), float(self.dice), float(self.optimize_bg),
                                     float(self.lovasz and self.lovasz_only_present)] + w))

    @property
    def weights(self):
        """The class weights on the device (a view of the settings buffer: in-place writes reach a captured graph)."""
        return self.cfg[4:]

    def set_border(self, weight, sigma=5.0):
        """The border term 1 + weight * exp(-(d1 + d2)^2 / (2 sigma^2)) on the CE of unlabelled pixels; weight 0 = off."""
        weight, sigma = float(weight), float(sigma)
        if weight < 0 or not sigma > 0:
            raise ValueError("border weight must not be negative and sigma must be positive, got %r, %r" % (weight, sigma))
        if weight > 0 and self.criterion == "Lovasz":
            raise ValueError("the border weight weighs the CE term: the Lovasz criterion has none (use CELovasz)")
        self.border_on, self.border_weight, self.border_sigma = weight > 0, weight, sigma
        self._set_legacy()
        self.border.copy_(torch.tensor([weight, sigma]))

    def _set_legacy(self):
        self.legacy = (self.K == 2 and self.criterion == "Multi" and self.class_weights is None and not self.optimize_bg
                       and not self.border_on)

    def set_border_values(self, weight, sigma=None):
        """In place: a captured step follows it (on / off is part of the step's configuration and stays)."""
        assert float(weight) > 0 and self.border_on, "the weight of a running border term; switch it with set_border()"
        sigma = self.border_sigma if sigma is None else float(sigma)
        assert sigma > 0
        self.border_weight, self.border_sigma = float(weight), sigma
        self.border.copy_(torch.tensor([float(weight), sigma]))

    def border_key(self):
        return self.border_on


class _EngineLib:
    """Engine.lib as it is at call time: tests and tracing scripts put a recorder in its place after construction."""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        return getattr(self._eng.lib, name)


class Network:
    def __init__(self, eng: Engine, use_instance_seg=True, n_classes=2):
        self.E = eng
        self.use_instance_seg = use_instance_seg
        self.n_classes = n_classes
        self.crit = SemCriterion(n_classes, eng.device)
        self.disc = DiscCriterion(eng.device)
        # the label-map operators of a step (border map, discriminative loss) answer in the step's arena; Engine.begin
        # puts another arena in place per configuration, hence the lookup at call time
        self.maps = LabelOps(eng.device, _EngineLib(eng), alloc=lambda shape, dtype: eng.arena.alloc(shape, dtype))

    # ------------------------------------------------------------------ blocks
    def block_v1(self, x: Act, pre: str, out: Act):
        """InvertedV1Residual (MobileNetDenseASPP.py:68-93): dw3x3-BN-ReLU6-pw-BN (+x)."""
        E = self.E
        cin = x.c
        cout = E.params.shapes[pre + ".conv.3.weight"][0]
        if E.block_v1_eval_fusable(x, cout):               # eval: the whole block in one launch, the dw output stays in LDS
            return E.block_v1_eval(x, pre, out, res=x if cin == cout else None)
        y1 = E.like(x, cin)
        if E.eval_fusable():                               # eval: BN.4 and the residual ride in the 1x1 conv's epilogue
            E.dwconv(x, pre + ".conv.0.weight", y1, stats=False)
            y1 = E.bn(y1, None, pre + ".conv.1", L.ACT_RELU6)
            return E.conv_bn_eval(y1, pre + ".conv.3.weight", out, pre + ".conv.4", L.ACT_NONE, res=x if cin == cout else None)
        _, s1 = E.dwconv(x, pre + ".conv.0.weight", y1, stats=True)
        y1 = E.bn(y1, s1, pre + ".conv.1", L.ACT_RELU6)
        y2 = E.like(x, cout)
        _, s2 = E.conv(y1, pre + ".conv.3.weight", y2, stats=True)
        return E.bn_out(y2, s2, pre + ".conv.4", L.ACT_NONE, out, res=x if cin == cout else None)

    def block_ir(self, x: Act, pre: str, out: Act, oscale=None):
        """InvertedResidual (MobileNetDenseASPP.py:96-123): pw-BN-ReLU6-dw-BN-ReLU6-pw-BN (+x).
        `oscale` folds a following Dropout2d (which scales the block output, residual included)
        into the materialising pass."""
        E = self.E
        cin = x.c
        chid = E.params.shapes[pre + ".conv.0.weight"][0]
        cout = E.params.shapes[pre + ".conv.6.weight"][0]
        y1 = E.like(x, chid)
        if E.eval_fusable() and oscale is None:
            # eval: expand conv stores ReLU6(BN(.)) (no prologue in the depthwise conv), the project conv applies BN.7 and
            # the residual in its epilogue (no materialising pass)
            E.conv_bn_eval(x, pre + ".conv.0.weight", y1, pre + ".conv.1", L.ACT_RELU6)
            y2 = E.like(x, chid)
            E.dwconv(y1, pre + ".conv.3.weight", y2, stats=False)
            y2 = E.bn(y2, None, pre + ".conv.4", L.ACT_RELU6)
            return E.conv_bn_eval(y2, pre + ".conv.6.weight", out, pre + ".conv.7", L.ACT_NONE, res=x if cin == cout else None)
        _, s1 = E.conv(x, pre + ".conv.0.weight", y1, stats=True)
        y1 = E.bn(y1, s1, pre + ".conv.1", L.ACT_RELU6)
        y2 = E.like(x, chid)
        _, s2 = E.dwconv(y1, pre + ".conv.3.weight", y2, stats=True)
        y2 = E.bn(y2, s2, pre + ".conv.4", L.ACT_RELU6)
        y3 = E.like(x, cout)
        _, s3 = E.conv(y2, pre + ".conv.6.weight", y3, stats=True)
        return E.bn_out(y3, s3, pre + ".conv.7", L.ACT_NONE, out, res=x if cin == cout else None,
                        oscale=oscale)

    def double_v1(self, x: Act, pre: str, out: Act):
        E = self.E
        cmid = E.params.shapes[pre + ".conv.down_conv_0.conv.3.weight"][0]
        mid = E.like(x, cmid)
        self.block_v1(x, pre + ".conv.down_conv_0", mid)
        return self.block_v1(mid, pre + ".conv.down_conv_1", out)

    # ------------------------------------------------------------------ backbone
    def unet(self, x_in: Act):
        """UNet.forward (unet_model.py:23-36).  x_in: [n,h,w,21] view (ld 24)."""
        E = self.E
        n, h, w = x_in.n, x_in.h, x_in.w
        widths = [(64, 32), (128, 64), (256, 128), (512, 256), (512, 512)]   # (buffer ld, x_k width)
        bufs = []
        for lvl, (ld, _) in enumerate(widths):
            bufs.append(E.new_act(n, h >> lvl, w >> lvl, ld, ld=ld))
        x1 = bufs[0].slice(0, 32)
        self.double_v1(x_in, "base.inc.conv", x1)
        feats = [x1]
        cur = x1
        for lvl in range(1, 5):
            cw = widths[lvl][1] // 2                       # conv half / pooled half
            pooled = bufs[lvl].slice(cw, cw)
            E.avgpool2(cur, pooled)
            self.double_v1(pooled, "base.down%d.mpconv" % lvl, bufs[lvl].slice(0, cw))
            cur = bufs[lvl].slice(0, 2 * cw)
            feats.append(cur)
        y = feats[4]
        for i, lvl in enumerate((3, 2, 1, 0)):
            pre = "base.up%d" % (i + 1)
            skip_w = widths[lvl][1]
            co = E.params.shapes[pre + ".up.weight"][1]
            up_dst = bufs[lvl].slice(skip_w, co)
            E.conv(y, pre + ".up.weight", up_dst, bias=pre + ".up.bias", transposed=True)
            cat = bufs[lvl].slice(0, skip_w + co)
            out = E.new_act(n, h >> lvl, w >> lvl, co)
            y = self.double_v1(cat, pre + ".conv", out)
        return y, feats

    # ------------------------------------------------------------------ heads
    def sem_head(self, x_dec: Act):
        """channelAttend (utils.py:402-420) + sem_seg_output (reseg.py:73-75,115-116)."""
        E = self.E
        P = E.params
        n, c = x_dec.n, x_dec.c
        mean = E.scratch(n * c)
        E.lib.isa_chan_mean(x_dec.d(), None, mean, E.st())
        hid, gate = E.f32(n * 16), E.f32(n * c)
        E.lib.isa_se_fc(mean, P.ptr("channelAttend.fc.0.weight"), P.ptr("channelAttend.fc.0.bias"),
                        P.ptr("channelAttend.fc.2.weight"), P.ptr("channelAttend.fc.2.bias"), n, c, 16, hid, gate, E.st())
        gated = x_dec.with_pro(Pro(bscale=gate))
        sem = E.new_act(n, x_dec.h, x_dec.w, self.n_classes)
        E.conv(gated, "sem_seg_output.weight", sem, bias="sem_seg_output.bias", record_bwd=False)
        reg = E.reg_conv("sem_seg_output.weight")
        if E.record:
            def bwd():
                # sem conv: weight/bias grads see x*gate; its data gradient is w.r.t. x*gate (dxa)
                dy = E.grads.grad_of(sem)
                E.lib.isa_conv_wgrad(gated.d(), gated.p(), dy.d(), P.gptr("sem_seg_output.weight"),
                                     P.gptr("sem_seg_output.bias"), L.IN_1X1, L.OUT_PLAIN, None, c, E.ws, E.ws.numel(),
                                     E.defer_handle(), E.st())
                dxa = E.new_act(n, x_dec.h, x_dec.w, c)
                E.lib.isa_conv_gemm(dy.d(), None, E.packer.ptr(reg["dgrad"]), reg["kp_d"], None, dxa.d(), L.IN_1X1,
                                    L.OUT_PLAIN, None, 0, E.st())
                dg, dmean = E.scratch(n * c), E.f32(n * c)
                acc = E.grads.claim(x_dec, E)
                E.lib.isa_se_bwd(dxa.d(), x_dec.d(), gate, hid, mean, P.ptr("channelAttend.fc.0.weight"),
                                 P.ptr("channelAttend.fc.2.weight"), 16, dg, dmean, P.gptr("channelAttend.fc.0.weight"),
                                 P.gptr("channelAttend.fc.0.bias"), P.gptr("channelAttend.fc.2.weight"),
                                 P.gptr("channelAttend.fc.2.bias"), E.grads.grad_of(x_dec).d(), acc, E.st())
            E.tape.append(bwd)
        return sem

    def _border_map(self, sem: Act, ins: torch.Tensor):
        """The step's border weight map fp32 [n,h,w] from its instance planes (either form forward() takes), in the arena."""
        if ins is None or ins.dim() != 4 or ins.numel() == 0:
            raise ValueError("the border weight is on: the step needs the batch's instance planes")
        lab, _ = self.maps.labels_from_planes(ins, "instance planes")
        assert lab.numel() == sem.n * sem.h * sem.w, "instance planes do not match the logits"
        return self.maps.border_map(lab.view(sem.n, sem.h, sem.w), self.crit.border)

    def sem_loss(self, sem: Act, sem_onehot: torch.Tensor, labels: torch.Tensor = None, ins: torch.Tensor = None):
        """Trainer-side semantic criterion on the logits (model.py:255-269), per self.crit: CE (weighted) and / or
        Dice (time=1, per class, fg or all), or Lovasz-Softmax with or without CE.  `labels`: the uint8 label map when
        the caller has it (compact targets), else taken from the one-hot.  Returns device tensor [ce, dice] (0 for a term
        the criterion lacks), [ce, 0, lovasz] for the Lovasz criteria; records d(sem).  With the border term on, `ins`
        (the batch's instance planes) gives the weight map of the CE term."""
        E = self.E
        n = sem.n
        if self.crit.legacy:             # the shipped criterion: its pinned 2-class kernels
            sums = E.scratch(8 * n)
            E.lib.isa_mask_loss_sums(sem.d(), None, sem_onehot, sums, E.st())
            coef, scal = E.f32(4 * n), E.f32(2)
            E.lib.isa_sem_loss(sums, n, coef, scal, E.st())
            if E.record:
                def bwd():
                    acc = E.grads.claim(sem, E)
                    E.lib.isa_mask_loss_grad(sem.d(), None, sem_onehot, coef, E.grads.grad_of(sem).d(), acc, E.st())
                E.tape.append(bwd)
            return scal
        K, cfg = sem.c, self.crit.cfg
        if labels is None:
            assert sem_onehot.dtype == torch.int64 and tuple(sem_onehot.shape) == (n, K, sem.h, sem.w)
            labels = self.maps.labels_from_onehot(sem_onehot)
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (n, sem.h, sem.w)
        pixw = self._border_map(sem, ins) if self.crit.border_on else None
        if self.crit.lovasz:
            return self._lovasz_loss(sem, labels, pixw)
        sums = E.scratch(3 * n * K + 2)
        self._k_sums(sem, labels, pixw, sums)
        coef, scal = E.f32(3 * n * K + 1), E.f32(2)
        E.lib.isa_sem_loss_k_assemble(sums, cfg, n, K, coef, scal, E.st())
        if E.record:
            def bwd():
                acc = E.grads.claim(sem, E)
                self._k_grad(sem, labels, pixw, coef, E.grads.grad_of(sem).d(), acc)
            E.tape.append(bwd)
        return scal

    def _k_sums(self, sem, labels, pixw, sums):
        E, cfg = self.E, self.crit.cfg
        if pixw is None:
            E.lib.isa_sem_loss_k_sums(sem.d(), labels, cfg, sums, E.st())
        else:
            E.lib.isa_sem_loss_k_sums_pw(sem.d(), labels, cfg, pixw, sums, E.st())

    def _k_grad(self, sem, labels, pixw, coef, dsem, acc):
        E, cfg = self.E, self.crit.cfg
        if pixw is None:
            E.lib.isa_sem_loss_k_grad(sem.d(), labels, cfg, coef, dsem, acc, E.st())
        else:
            E.lib.isa_sem_loss_k_grad_pw(sem.d(), labels, cfg, coef, pixw, dsem, acc, E.st())

    def _lovasz_loss(self, sem: Act, labels: torch.Tensor, pixw: torch.Tensor = None):
        """CELovasz: the CE term from the K-class kernels as they are, then the Lovasz-Softmax launches (keys, segmented
        sort, coefficients per class group; one assemble); the backward adds both gradients into d(sem).  The launch
        count depends on (K, B, H*W, per_image) alone and nothing is read back: the step captures."""
        E, crit = self.E, self.crit
        n, K, hw, cfg = sem.n, sem.c, sem.h * sem.w, self.crit.cfg
        T = L.SEGSORT_TILE
        per_image = int(crit.lovasz_per_image)
        nimg = n if per_image else 1
        seglen = n * hw // nimg
        ntiles = (seglen + T - 1) // T
        if K * n * hw >= 1 << 31:
            raise L.IsaError("Lovasz criterion: K*B*H*W = %d elements, the segmented sort takes fewer than 2^31" % (K * n * hw))
        scal = E.arena.alloc((3,), torch.float32, zero=True)
        coef = None
        if crit.ce:
            sums = E.scratch(3 * n * K + 2)
            self._k_sums(sem, labels, pixw, sums)
            coef = E.f32(3 * n * K + 1)
            E.lib.isa_sem_loss_k_assemble(sums, cfg, n, K, coef, scal, E.st())
        record = E.record
        G = E.scratch(K * nimg).view(torch.int32)                       # zero at step start: the keys kernel adds to it
        partial = E.arena.alloc((K * nimg * ntiles,), torch.float64)
        gpix = E.f32(K * n * hw) if record else None
        kg = lovasz_class_group(K, n * hw, record)
        u32 = [E.arena.alloc((kg * n * hw,), torch.int32) for _ in range(6)]
        k_in, v_in, k_out, v_out, k_tmp, v_tmp = u32
        table = E.arena.alloc((L.segsort_table_elems(kg * nimg, seglen),), torch.int32)
        tcnt = E.arena.alloc((kg * nimg * ntiles,), torch.int32)
        for c0 in range(0, K, kg):
            nc = min(kg, K - c0)
            s0 = c0 * nimg
            E.lib.isa_lovasz_keys(sem.d(), labels, c0, nc, per_image, k_in, v_in, G[s0:], E.st())
            E.lib.isa_segsort_kv_u32(k_in, v_in, k_out, v_out, nc * nimg, seglen, 0, 30, k_tmp, v_tmp, table, table.numel(),
                                     E.st())
            E.lib.isa_lovasz_coef(k_out, v_out, G[s0:], nc * nimg, seglen, tcnt, partial[s0 * ntiles:],
                                  gpix[s0 * seglen:] if record else None, E.st())
        segloss = E.arena.alloc((K * nimg,), torch.float64)
        scale = E.f32(K * nimg)
        E.lib.isa_lovasz_assemble(partial, G, cfg, n, K, per_image, hw, segloss, scale, scal[2:], E.st())
        if record:
            def bwd():
                acc = E.grads.claim(sem, E)
                dsem = E.grads.grad_of(sem).d()
                if coef is not None:
                    self._k_grad(sem, labels, pixw, coef, dsem, acc)
                    acc = 1
                E.lib.isa_lovasz_grad(sem.d(), gpix, scale, per_image, dsem, acc, E.st())
            E.tape.append(bwd)
        return scal

    def onehot_map(self, sem_onehot: torch.Tensor) -> torch.Tensor:
        """int64 one-hot [n,K,h,w] -> fp32 argmax(1) map [n, h*w] (sem_seg_argmax of reseg.py:118, on the device)."""
        E = self.E
        n, c, h, w = sem_onehot.shape
        assert c == self.n_classes and sem_onehot.dtype == torch.int64
        out = E.f32(n, h * w)
        if c == 2:
            E.lib.isa_onehot_map(sem_onehot, n, h * w, out, E.st())
        else:
            E.lib.isa_labels_from_onehot(sem_onehot, n, c, h * w, None, out, E.st())
        return out

    def softmax_nchw(self, logits: Act) -> torch.Tensor:
        out = torch.empty((logits.n, logits.c, logits.h, logits.w), dtype=torch.float32, device=logits.buf.device)
        self.E.lib.isa_softmax_nchw(logits.d(), out, self.E.st())
        return out

    def argmax_map(self, logits: Act):
        E = self.E
        out = E.new_act(logits.n, logits.h, logits.w, 1)
        E.lib.isa_chan_argmax(logits.d(), out.d(), E.st())
        return out

    def class_map(self, sem: Act) -> torch.Tensor:
        """uint8 class ids [n,h,w] of the logits `sem` on the device (isa_sem_confusion without labels): the arg-max over
        the K channels, first maximum wins, NaN is the maximum.  A new tensor, not arena memory."""
        E = self.E
        out = torch.empty((sem.n, sem.h, sem.w), dtype=torch.uint8, device=sem.buf.device)
        E.lib.isa_sem_confusion(sem.d(), None, sem.c, None, None, out, E.st())
        return out

    def sem_confusion(self, sem: Act, labels: torch.Tensor):
        """(conf int64 [n,K,K], oob int32 [n]) of the logits `sem` against the uint8 label map [n,h,w] in one pass over
        the logits: conf[i][t][p] pixels of image i with label t and predicted class p; labels >= K go to oob[i]."""
        E = self.E
        K = sem.c
        assert labels.dtype == torch.uint8 and labels.is_contiguous() and labels.numel() == sem.n * sem.h * sem.w
        conf = torch.empty((sem.n, K, K), dtype=torch.int64, device=sem.buf.device)
        oob = torch.empty((sem.n,), dtype=torch.int32, device=sem.buf.device)
        E.lib.isa_sem_confusion(sem.d(), labels, K, conf, oob, None, E.st())
        return conf, oob

    # ------------------------------------------------------------------ boundary
    def to_nhwc(self, x: torch.Tensor, c_pad=None) -> Act:
        """NCHW fp32 (reference layout) -> NHWC activation view."""
        E = self.E
        n, c, h, w = x.shape
        x = x.contiguous()
        dst = E.new_act(n, h, w, c, ld=rup(c, 8))
        dst.needs_grad = False
        self._keep = x
        E.lib.isa_nchw_to_nhwc(x, c, dst.d(), E.st())
        return dst

    def image_ex(self, rgb: torch.Tensor) -> Act:
        """uint8 RGB [n,h,w,3] -> the 21-channel standardized NHWC input (ImageEx + ToTensor + Standardization,
        lib/utils.py:90-113, preprocess.py:192-195) in one kernel; replaces the six skimage conversions per image
        of the reference's data pipeline (parity unpinned, see oracle/image_ex_ref.py)."""
        E = self.E
        assert rgb.dtype == torch.uint8 and rgb.dim() == 4 and rgb.shape[-1] == 3, "expects uint8 [n,h,w,3]"
        n, h, w, _ = rgb.shape
        rgb = rgb.to(E.device).contiguous()
        dst = E.new_act(n, h, w, 21, ld=24)
        dst.needs_grad = False
        self._keep = rgb
        E.lib.isa_image_ex(rgb, dst.d(), E.st())
        return dst

    def input_view(self, x: torch.Tensor) -> Act:
        """Network input: the reference's [n,21,h,w] float tensor, or raw uint8 RGB [n,h,w,3] expanded on device."""
        if x.dtype == torch.uint8:
            return self.image_ex(x)
        return self.to_nhwc(x.to(device=self.E.device, dtype=torch.float32))

    def collate_targets(self, sem: torch.Tensor, ins: torch.Tensor, labels=False, onehot=True):
        """Targets as the reference's collate function leaves them before its last five lines (dataset.py:349-379):
        ins uint8 [n,h,w,K] instance planes, sem uint8 [n,h,w] -> (sem one-hot int64 [n,C,h,w], ins int64 [n,K,h,w])
        on the device (isa_collate_targets; isa_collate_targets_k for C = n_classes > 2).  8.6x less PCIe traffic than
        shipping the int64 tensors.  labels=True: also the uint8 label map for the K-class criterion, returned third;
        onehot=False then skips the one-hot (None in its place)."""
        E = self.E
        assert ins.dtype == torch.uint8 and ins.dim() == 4 and sem.dtype == torch.uint8 and sem.dim() == 3
        n, h, w, k = ins.shape
        assert tuple(sem.shape) == (n, h, w)
        ins, sem = ins.to(E.device).contiguous(), sem.to(E.device).contiguous()
        C = self.n_classes
        ins_out = E.arena.alloc((n, k, h, w), torch.int64)
        sem_out = E.arena.alloc((n, C, h, w), torch.int64) if onehot or not labels else None
        if C == 2 and not labels:
            E.lib.isa_collate_targets(ins, sem, n, h, w, k, ins_out, sem_out, E.st())
            return sem_out, ins_out
        lab = E.arena.alloc((n, h, w), torch.uint8) if labels else None
        E.lib.isa_collate_targets_k(ins, sem, n, h, w, k, C, ins_out, sem_out, lab, E.st())
        return (sem_out, ins_out, lab) if labels else (sem_out, ins_out)

    def to_nchw(self, a: Act) -> torch.Tensor:
        E = self.E
        out = torch.empty((a.n, a.c, a.h, a.w), dtype=torch.float32, device=a.buf.device)
        E.lib.isa_nhwc_to_nchw(a.d(), out, E.st())
        return out
