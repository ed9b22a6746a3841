"""Drop-in `ReSeg` (reference: code/lib/archs/reseg.py:52-130).

Same constructor signature, same `forward(training, *_input)` contract, same `state_dict()` keys,
shapes and order (891 tensors), `.base` attribute, `.parameters()`, `.train()/.eval()`, `.cuda()`.
All compute runs in the HIP library behind include/isa_kernels.h; this class only owns the
parameters (views into one flat fp32 buffer, so DDP needs one all-reduce and the optimizer one
kernel) and sequences launches.  Missing library or missing GPU => hard error, never a fallback.
"""
import torch
import torch.nn as nn

from . import lib as L
from .engine import Engine, ParamStore
from .network import Network
from .instance_head import InstanceHead
from .schema import state_dict_schema

# the columns of ReSeg.instance_properties (isa_instance_props, include/isa_kernels.h)
PROPS_COLUMNS = ("area", "x0", "y0", "x1", "y1", "centroid_x", "centroid_y", "mu_xx", "mu_yy", "mu_xy", "major_axis",
                 "minor_axis", "eccentricity", "orientation", "perimeter", "touches_border", "extent", "equivalent_diameter",
                 "compactness", "first_pixel", "mean_c0", "mean_c1", "mean_c2", "mean_c3")


class _Node(nn.Module):
    """Anonymous container reproducing the reference's module tree for state_dict naming."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("container node: compute lives in the HIP engine")


class ReSeg(nn.Module):
    def __init__(self, n_classes, use_instance_seg=True, pretrained=True, use_coordinates=False,
                 use_wae=True, usegpu=True, training=True, dtype=torch.float32, device=None):
        super().__init__()
        if not 2 <= n_classes <= 32:
            raise ValueError("n_classes must be in [2, 32] (the K-class criterion kernels), got %d" % n_classes)
        if use_instance_seg and n_classes != 2:
            # the instance head reads sem_seg_argmax as a {0,1} foreground mask (reseg.py:118-123)
            raise ValueError("the instance head needs n_classes == 2 (foreground / background); build "
                             "ReSeg(n_classes, use_instance_seg=False) for a K-class semantic network")
        if not torch.cuda.is_available():
            raise RuntimeError("ReSeg (MI355X build) needs a GPU: there is no CPU fallback")
        L.lib()                                   # fail loudly if the HIP library is missing
        self.backbone = "Unet"
        self.n_classes = n_classes
        self.use_instance_seg = use_instance_seg
        self.use_wae = use_wae
        self.compute_dtype = dtype
        dev = torch.device(device or "cuda")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.store = ParamStore(state_dict_schema(use_instance_seg, n_classes), dev)
        self._build_tree()
        self.engine = Engine(self.store, dtype, dev)
        self.net = Network(self.engine, use_instance_seg, n_classes)
        self.head = InstanceHead(self.net)
        self.reset_parameters()
        self.train(training)

    # ------------------------------------------------------------------ module tree
    def _build_tree(self):
        st = self.store
        self._nbt = {}
        for name in st.names:
            parts = name.split(".")
            mod = self
            for p in parts[:-1]:
                if p not in mod._modules:
                    mod.add_module(p, _Node())
                mod = mod._modules[p]
            leaf = parts[-1]
            if leaf == "num_batches_tracked":
                buf = torch.zeros((), dtype=torch.long)
                mod.register_buffer(leaf, buf)
                self._nbt[name] = (mod, leaf)
            elif leaf in ("running_mean", "running_var"):
                mod.register_buffer(leaf, st.view(name))
            else:
                p_ = nn.Parameter(st.view(name))
                p_.grad = st.gview(name)
                mod.register_parameter(leaf, p_)

    def reset_parameters(self, seed=None):
        """Fresh weights in the spirit of torch defaults (kaiming-uniform convs, BN gamma=1/beta=0,
        maskBN gamma~U(0,1) as utils.py:561).  Host-side plumbing on the flat buffer views."""
        g = torch.Generator(device="cpu")
        g.manual_seed(0 if seed is None else int(seed))
        st = self.store
        bn_prefixes = {n[:-len(".running_mean")] for n in st.names if n.endswith(".running_mean")}
        for name in st.names:
            if name in st.int_buffers:
                continue
            v, shape = st.view(name), st.shapes[name]
            prefix, leaf = name.rsplit(".", 1)
            if leaf == "running_mean":
                v.zero_()
            elif leaf == "running_var":
                v.fill_(1.0)
            elif prefix in bn_prefixes and leaf == "weight":
                v.copy_(torch.rand(shape, generator=g)) if prefix == "decoder.attend.bn" else v.fill_(1.0)
            elif prefix in bn_prefixes and leaf == "bias":
                v.zero_()
            else:
                fan_in = 1
                for d in (shape[1:] if len(shape) > 1 else shape):
                    fan_in *= d
                if leaf == "bias":                       # conv/linear bias: fan-in of its weight
                    wshape = st.shapes.get(prefix + ".weight", shape)
                    fan_in = 1
                    for d in wshape[1:]:
                        fan_in *= d
                bound = (1.0 / max(fan_in, 1)) ** 0.5
                v.copy_((torch.rand(shape, generator=g) * 2 - 1) * bound)

    # ------------------------------------------------------------------ nn.Module plumbing
    def _apply(self, fn, recurse=True):
        # parameters are views of one flat device buffer; moving/casting them individually would
        # break that.  `.cuda()` / `.to(same device)` are accepted as no-ops like the reference's
        # `model.cuda()` call site (model.py:52).
        probe = fn(torch.empty(0, device=self.store.device))
        if probe.device != self.store.device or probe.dtype != torch.float32:
            raise RuntimeError("ReSeg parameters live in one flat fp32 GPU buffer; cannot move/cast")
        return self

    def state_dict(self, *args, **kwargs):
        for name, (mod, leaf) in self._nbt.items():
            mod._buffers[leaf].fill_(self.store.int_buffers[name])
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, strict=True):
        out = super().load_state_dict(state_dict, strict=strict)
        for name, (mod, leaf) in self._nbt.items():
            self.store.int_buffers[name] = int(mod._buffers[leaf])
        self.engine.packer.table = None if self.engine.packer.entries else self.engine.packer.table
        self._weights_dirty = True
        self.engine.eval_bn_stale = True
        return out

    def mark_weights_dirty(self):
        """Call after an optimizer step changed the flat parameter buffer (repack on next forward)."""
        self._weights_dirty = True
        self.engine.eval_bn_stale = True

    # ------------------------------------------------------------------ hipGraph-replayed GT-free inference
    def infer_graphed(self, x):
        """(sem_out, sem_argmax) = forward(False, x) replayed from a hipGraph (pred_list-style batched inference:
        ~70 launches per batch are launch-bound at bs=16).  One graph per input shape/dtype; the first call of a
        shape runs eagerly, the second captures.  Returned tensors are the graph's static outputs: consume or
        copy them before the next call."""
        assert not self.training, "infer_graphed is for eval mode (running BatchNorm statistics)"
        dev = self.store.device
        key = (tuple(x.shape), x.dtype)
        graphs = self.__dict__.setdefault("_infer_graphs", {})
        slot = graphs.get(key)
        if slot is None:
            graphs[key] = dict(state="warm")
            with torch.no_grad():
                return self.forward(False, x, _arena_key=("infer_graph",) + key)
        if slot["state"] == "eager":
            with torch.no_grad():
                return self.forward(False, x)
        if slot["state"] == "warm":
            slot["x"] = torch.empty(tuple(x.shape), dtype=x.dtype if x.dtype == torch.uint8 else torch.float32, device=dev)
            slot["x"].copy_(x, non_blocking=True)
            if getattr(self, "_weights_dirty", True) and self.engine.packer.entries:
                self.engine.packer.pack()                  # weights are constant across replays: pack outside
                self._weights_dirty = False
            if self.engine.eval_bn_stale:
                self.engine.refresh_eval_bn()              # ... and so are the eval-mode BN constants
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"), torch.no_grad():
                    out = self.forward(False, slot["x"], _arena_key=("infer_graph",) + key)
                self.engine.freeze_arena()
            except Exception as e:
                import sys
                print("[isa_amd] hipGraph capture failed (%s: %s); inference runs eagerly" % (type(e).__name__, e),
                      file=sys.stderr, flush=True)
                torch.cuda.synchronize()
                slot["state"] = "eager"
                with torch.no_grad():
                    return self.forward(False, x)
            slot.update(state="ready", graph=g, out=out)
        else:
            if getattr(self, "_weights_dirty", False):     # parameters changed since capture: repack, then replay
                self.engine.packer.pack()
                self._weights_dirty = False
            if self.engine.eval_bn_stale:                  # same buffers the graph reads, recomputed in place
                self.engine.refresh_eval_bn()
            slot["x"].copy_(x, non_blocking=True)
        slot["graph"].replay()
        return slot["out"]

    def set_criterion(self, criterion="Multi", class_weights=None, optimize_bg=False, lovasz_per_image=False,
                      lovasz_only_present=False):
        """The semantic criterion of training steps and sem_costs (Model.__define_criterion, model.py:102-133); "Lovasz" and
        "CELovasz" add lovasz_softmax (losses/lovasz_losses.py:156-196) with its per_image / only_present options."""
        self.net.crit.set(criterion, class_weights, optimize_bg, lovasz_per_image, lovasz_only_present)

    def sem_costs(self, sem_seg_target, ins=None):
        """Semantic criterion (set_criterion; default CE + Dice(time=1)) of the LAST forward's logits against a one-hot
        int64 target [B,K,H,W] (validation branch of model.py:244-270).  Returns a device tensor [ce, dice] (0 for a
        term the criterion lacks; [ce, 0, lovasz] for the Lovasz criteria); must be called before the next forward (the
        logits live in that step's arena).  ins: the batch's instance planes, needed when the border term is on."""
        sem = getattr(self, "_last_sem", None)
        assert sem is not None, "sem_costs() follows a forward()"
        t = sem_seg_target.to(self.store.device).contiguous()
        assert t.dtype == torch.int64 and tuple(t.shape) == (sem.n, self.n_classes, sem.h, sem.w)
        was = self.engine.record
        self.engine.record = False
        try:
            if ins is not None:
                ins = ins.to(self.store.device).contiguous()
            return self.net.sem_loss(sem, t, None, ins).clone()
        finally:
            self.engine.record = was

    # ------------------------------------------------------------------ ground-truth-free instance inference
    def segment(self, x, max_objects=32, *, sem_map=None, injected_s_t=None, capture=None):
        """(sem_out, sem_argmax, labels, n_objects) for images `x` (either input form of forward) without ground truth:
        labels uint8 [B,H,W] (0 = background or unexplained foreground, 1..n_objects[b] = instances in the order they
        were found), n_objects int32 [B], both on the device.  One glimpse point per object - the arg-max of the
        hard-attention score map over the foreground no instance has claimed yet - and one decoder pass per point;
        the instance takes the unclaimed pixels its full-resolution prediction calls foreground, and its point
        (InstanceHead.segment; DESIGN.md "Instance inference").  Stops when every image is explained or after
        `max_objects` (1..255) instances per image.  Eval mode only.
        sem_map (fp32 {0,1} [B,H*W]) replaces the predicted foreground; injected_s_t (list of int32 device vectors)
        replaces the point of iteration t and fixes the iteration count to its length; capture receives `merge` and per
        iteration `it%d.s_t` and `it%d.L%d.pred`, the names forward uses."""
        assert not self.training, "segment is for eval mode (running BatchNorm statistics, no Dropout2d)"
        if not self.use_instance_seg:
            raise RuntimeError("segment() needs a model built with use_instance_seg=True")
        max_objects = int(max_objects)
        if not 1 <= max_objects <= 255:
            raise ValueError("max_objects must be in 1..255 (labels are uint8), got %d" % max_objects)
        net = self.net
        dev = self.store.device
        with torch.no_grad():
            x_dec, feats, B, H, W = self._backbone(x, "segment")
            sem = net.sem_head(x_dec)
            self._last_sem = sem
            sem_out = net.to_nchw(sem)
            sem_argmax = net.to_nchw(net.argmax_map(sem))
            if sem_map is None:
                fg = sem_argmax.reshape(B, -1)
            else:
                fg = sem_map.to(device=dev, dtype=torch.float32).reshape(B, -1).contiguous()
                assert fg.shape[1] == H * W, "sem_map must be [B, H*W]"
            if injected_s_t is not None:
                injected_s_t = [v.to(device=dev, dtype=torch.int32).contiguous() for v in injected_s_t]
                assert all(v.numel() == B for v in injected_s_t)
            labels, count = self.head.segment(x_dec, feats, fg, max_objects, injected_s_t, capture)
            return sem_out, sem_argmax, labels.clone(), count.clone()    # (the state lives in the step's arena)

    # ------------------------------------------------------------------ scoring instance predictions on the device
    def _label_map(self, planes, what):
        """uint8 label map [B, H*W] of ground-truth planes in either form forward() takes (isa_labels_from_planes)."""
        t = planes.to(self.store.device).contiguous()
        assert t.dim() == 4, "%s must be uint8 [B,H,W,K] or int64 [B,K,H,W]" % what
        out, k = self.net.labels_from_planes(t, what, self._new)
        return out.view(out.shape[0], -1), k

    def _new(self, shape, dtype):
        """The allocator of the calls that answer in new tensors, not in a step's arena."""
        return torch.empty(shape, dtype=dtype, device=self.store.device)

    def _pair_scores(self, a, b, na, nb, n_a, n_b, oob):
        """[B,8] scores (isa_instance_scores) of the uint8 maps a, b [B, L]; the out-of-range counts go to oob [B]."""
        E = self.engine
        n, Lp = a.shape
        if not (1 <= na <= 256 and 1 <= nb <= 256 and na * nb <= 16384):
            raise ValueError("label ids: %d x %d counters; each side at most 256 and the product at most 16384" % (na, nb))
        hist = torch.empty((n, na, nb), dtype=torch.int32, device=a.device)
        out = torch.empty((n, 8), dtype=torch.float64, device=a.device)
        E.lib.isa_label_pair_hist(a, b, n, Lp, na, nb, hist, oob, L.HIST_AGGREGATE, E.st())
        E.lib.isa_instance_scores(hist, n, na, nb, n_a, n_b, out, E.st())
        return out

    def score_instances(self, labels, n_objects, ins_target, n_target, sem_argmax=None, sem_target=None, *,
                        max_objects=255, check=True):
        """Scores of predicted label maps (segment's `labels` uint8 [B,H,W] and `n_objects` int32 [B]) against the ground
        truth, on the device: a double tensor [B,8] whose columns are
          0 best Dice ground truth -> prediction, 1 best Dice prediction -> ground truth, 2 Symmetric Best Dice,
          3 objects present in the ground truth, 4 objects present in the prediction, 5 |n_target - n_objects| (|DiC|),
          6 foreground Dice, 7 zero
        (calc_bd / calc_sbd / calc_dic / calc_dice of evaluate.py, from one joint histogram per image: isa_label_pair_hist,
        isa_instance_scores).  ins_target: the instance planes in either form forward() takes (uint8 [B,H,W,K] or int64
        [B,K,H,W]); where planes overlap the first one gets the pixel.  n_target: the ground-truth object counts [B] or
        [B,1].  Column 6 compares sem_argmax (segment's fp32 [B,1,H,W]) with the foreground of sem_target (uint8 [B,H,W] or
        one-hot int64 [B,C,H,W]) when both are given, and the foregrounds of the two label maps otherwise.
        max_objects: the largest label the prediction can hold (segment's cap).  (K + 1) * (max_objects + 1) counters must
        not exceed 16384; a pixel whose label lies outside is not scored, and with check=True (one device read, the only
        host synchronisation of the call) that raises ValueError - there is no other path for such maps; with check=False
        the counts stay on the device in self.last_score_oob (int32 [2,B]) for the caller to read.
        Empty maps: column 0 is NaN for a ground truth without objects and 0.0 when only the prediction has none (column
        1 mirrors it), so SBD is NaN when both are empty and 0.0 when one is - where evaluate.calc_bd raises ValueError,
        which the device cannot; column 6 is NaN when both foregrounds are empty."""
        dev = self.store.device
        with torch.no_grad():
            labels = labels.to(dev)
            assert labels.dtype == torch.uint8 and labels.dim() == 3, "labels: uint8 [B,H,W]"
            B = labels.shape[0]
            pred = labels.contiguous().view(B, -1)
            if pred.shape[1] % 4:
                raise ValueError("H*W must be a multiple of 4, got %d" % pred.shape[1])
            gt, k = self._label_map(ins_target, "ins_target")
            assert tuple(gt.shape) == tuple(pred.shape), "ins_target and labels differ in size"
            n_pred = n_objects.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            n_gt = n_target.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            assert n_pred.numel() == B and n_gt.numel() == B
            oob = torch.empty((2, B), dtype=torch.int32, device=dev)
            out = self._pair_scores(gt, pred, k + 1, int(max_objects) + 1, n_gt, n_pred, oob[0])
            limits = ["ground-truth labels 0..%d, predicted labels 0..%d" % (k, int(max_objects))]
            if sem_argmax is not None and sem_target is not None:
                fg_pred, _ = self._label_map(sem_argmax.to(dev).float().reshape(B, 1, 1, -1), "sem_argmax")
                st = sem_target.to(dev).contiguous()
                if st.dtype == torch.uint8:
                    assert st.dim() == 3, "compact sem_target: uint8 [B,H,W]"
                    fg_gt, nc = st.view(B, -1), self.n_classes
                else:
                    assert st.dtype == torch.int64 and st.dim() == 4, "sem_target: one-hot int64 [B,C,H,W]"
                    nc = st.shape[1]
                    fg_gt = self.net.labels_from_onehot(st, self._new).view(st.shape[0], -1)
                assert tuple(fg_gt.shape) == tuple(pred.shape) == tuple(fg_pred.shape)
                sem = self._pair_scores(fg_gt, fg_pred, nc, 2, None, None, oob[1])
                out[:, 6].copy_(sem[:, 6])
                limits.append("semantic classes 0..%d" % (nc - 1))
            else:
                oob[1].zero_()
            self.last_score_oob = oob                     # for callers that pass check=False and read it with their own copy
            if check:
                bad = oob.cpu()
                for row, limit in zip(bad, limits):
                    if int(row.sum()):
                        raise ValueError("score_instances: %d pixels of images %s carry a label outside the histogram (%s); "
                                         "at most 256 ids a side and 16384 pairs are counted"
                                         % (int(row.sum()), torch.nonzero(row).view(-1).tolist(), limit))
            return out

    # ------------------------------------------------------------------ discriminative embedding loss
    def _emb_act(self, emb):
        """(Act, emb was one already) of an embedding: an engine Act as it is, fp32 or bf16 [B,C,H,W] copied into NHWC."""
        from .engine import Act, rup
        as_act = isinstance(emb, Act)
        if as_act:
            a = emb
        else:
            dev = self.store.device
            t = emb.to(dev)
            if t.dim() != 4 or t.dtype not in (torch.float32, torch.bfloat16):
                raise TypeError("emb: fp32 or bf16 [B,C,H,W] or an engine Act, got %s %s" % (t.dtype, tuple(t.shape)))
            B, C, H, W = t.shape
            buf = torch.zeros((B, H, W, rup(C, 8)), dtype=t.dtype, device=dev)
            buf[..., :C].copy_(t.permute(0, 2, 3, 1))
            a = Act(buf, 0, C)
        if not 1 <= a.c <= 32:
            raise ValueError("emb: 1..32 channels, got %d" % a.c)
        return a, as_act

    def discriminative_loss(self, emb, ins, n_objects, delta_var=0.5, delta_dist=1.5, norm=2, form='reference',
                            weights=None, unit_means=None, grad=False):
        """The discriminative (pull / push) loss of an instance embedding, on the device (DiscriminativeLoss,
        losses/discriminative.py:162-213; isa_disc_*).  emb: float [B,C,H,W] (fp32 or bf16, C <= 32)
        or an engine Act; ins: the instance planes in any form isa_labels_from_planes takes (uint8 [B,H,W,K], int64 or fp32
        [B,K,H,W], K <= 32; overlapping planes: the first one gets the pixel) or a ready uint8 label map [B,H,W] (0 =
        background, i + 1 = plane i); n_objects [B] or [B,1]: planes past it are ignored by the means and the var / dist /
        reg terms and stay foreground for qreg.  form 'reference' = var + 0.005 qreg on unit-length means (what the
        reference's discriminative_loss computes), 'full' = var + dist + 0.001 reg on plain means; weights = (alpha, beta,
        gamma, gamma_q) and unit_means override the form's.  Returns a dict of device tensors: loss, var, dist, reg, qreg
        (scalars) and means [B,K,C]; with grad=True also grad = d loss / d emb, shaped like emb (an Act for an Act).  Nothing
        is read back: the call does not synchronise."""
        from .engine import Act
        from .network import DiscCriterion
        dev = self.store.device
        with torch.no_grad():
            a, as_act = self._emb_act(emb)
            lab = ins.to(dev).contiguous()
            if lab.dtype == torch.uint8 and lab.dim() == 3:
                labels, k = lab.view(lab.shape[0], -1), L.DISC_MAX_K
            else:
                labels, k = self._label_map(lab, "ins")
            if not 1 <= k <= L.DISC_MAX_K:
                raise ValueError("ins: 1..32 planes, got %d" % k)
            assert tuple(labels.shape) == (a.n, a.h * a.w), "ins and emb differ in size"
            n_obj = n_objects.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            assert n_obj.numel() == a.n
            crit = DiscCriterion(dev)
            crit.set(1.0, delta_var, delta_dist, norm, form, weights, unit_means)
            scal, mu, gfn = self.net.disc_loss(a, labels, k, n_obj, crit.cfg, crit.norm, self._new)
            out = dict(loss=scal[0], var=scal[1], dist=scal[2], reg=scal[3], qreg=scal[4], means=mu[:, :k, :a.c])
            if grad:
                g = Act(torch.empty_like(a.buf), a.c0, a.c)
                gfn(g, 0)
                out["grad"] = g if as_act else g.buf[..., :a.c].permute(0, 3, 1, 2)
            return out

    # ------------------------------------------------------------------ clustering the instance embedding into instances
    def _backbone(self, x, key):
        """Eval-mode backbone on `x` (either input form of forward): (x_dec, feats, B, H, W)."""
        assert not self.training, "eval mode only (running BatchNorm statistics)"
        if not self.use_instance_seg:
            raise RuntimeError("the instance embedding needs a model built with use_instance_seg=True")
        if x.dtype == torch.uint8:
            assert x.dim() == 4 and x.shape[3] == 3, "uint8 input must be RGB [B,H,W,3]"
            B, H, W = x.shape[0], x.shape[1], x.shape[2]
        else:
            assert x.dim() == 4 and x.shape[1] == 21, "expects [B,21,H,W] (ImageEx tensor, utils.py:109)"
            B, H, W = x.shape[0], x.shape[2], x.shape[3]
        assert H % 16 == 0 and W % 16 == 0
        x_dec, feats = self._eval_unet(x, key)
        return x_dec, feats, B, H, W

    def _eval_unet(self, x, key):
        """Starts an eval-mode step in the arena of (key, x's shape and dtype), repacks weights that changed and runs the
        backbone on `x`: (x_dec, feats).  Asks nothing of the model's heads; the caller has checked for eval mode."""
        E, net = self.engine, self.net
        E.begin(bn_train=False, record=False, key=(key, tuple(x.shape), x.dtype))
        if getattr(self, "_weights_dirty", True) and E.packer.entries:
            E.packer.pack()
        self._weights_dirty = False
        return net.unet(net.input_view(x))

    def embedding(self, x):
        """The instance embedding x_enc float32 [B,24,H,W] of images `x` (either input form of forward) from the eval-mode
        network: backbone, then ins_seg_output_1 / ins_seg_output_2 (reseg.py:78-102) - what the discriminative loss is
        trained on and what cluster_embedding clusters.  Needs no ground truth."""
        with torch.no_grad():
            x_dec, _, _, _, _ = self._backbone(x, "embedding")
            return self.net.to_nchw(self.head.stems(x_dec))

    def cluster_embedding(self, emb, fg, *, method='meanshift', bandwidth=None, delta_var=0.5, delta_dist=1.5, shifts=3,
                          max_objects=32, min_pixels=1, assign_rest=True, refine=0, n_objects=None, iters=10,
                          init='farthest', max_rounds=None):
        """Clusters an instance embedding into instances, per image, on the device (isa_cluster_*).
        emb: float [B,C,H,W] (fp32 or bf16, C <= 32) or an engine Act; fg: [B,H,W] or [B,H*W] of any dtype, non-zero =
        foreground.  Distances are squared Euclidean, evaluated as sum_j (x[j] - c[j])^2 in fp32.
        method 'meanshift' (no object count needed): greedy flat-kernel mean-shift.  The first free foreground pixel seeds a
        centre, `shifts` (0..8) times the centre moves to the mean of the free pixels within `bandwidth`, those pixels become
        an instance if they are at least min_pixels (else noise), until nothing is free or max_objects (1..32) instances
        exist; with assign_rest what is left takes the label of its nearest centre.  The launch sequence is fixed, so the
        loop also ends after max_rounds rounds (default max_objects, at most 256), and a ball refused as noise uses up a
        round like an object does: with min_pixels = 1 nothing is refused and the budget never binds; with min_pixels > 1
        pass max_rounds = max_objects + the refused balls to allow for.  bandwidth=None: delta_dist, the middle
        of the admissible interval [2 delta_var, 2 delta_dist - 2 delta_var) of an embedding at zero var and dist loss.
        refine=r then runs r Lloyd iterations from the centres found, over the whole foreground.
        method 'kmeans': n_objects [B] clusters per image (at most the foreground pixels and max_objects), `iters` (0..64)
        Lloyd iterations from init='farthest' (deterministic maximin from the first foreground pixel) or a tensor [B,K,C].
        Returns a dict of device tensors: labels uint8 [B,H,W] (0 background, 1..n in the order of the centres), n_objects
        int32 [B], centres float32 [B,32,C], sizes int32 [B,32], moved int32 [B] (k-means: pixels whose label changed in the
        last iteration).  Bit-reproducible; nothing is read back: the call does not synchronise and can be captured."""
        if method not in ('meanshift', 'kmeans'):
            raise ValueError("method must be 'meanshift' or 'kmeans', got %r" % (method,))
        max_objects, shifts, iters, refine, min_pixels = int(max_objects), int(shifts), int(iters), int(refine), int(min_pixels)
        if not 1 <= max_objects <= L.DISC_MAX_K:
            raise ValueError("max_objects must be in 1..32, got %d" % max_objects)
        if not 0 <= shifts <= L.CLUSTER_MAX_SHIFTS:
            raise ValueError("shifts must be in 0..8, got %d" % shifts)
        if not 0 <= iters <= L.CLUSTER_MAX_ITERS or not 0 <= refine <= L.CLUSTER_MAX_ITERS:
            raise ValueError("iters and refine must be in 0..64, got %d and %d" % (iters, refine))
        if min_pixels < 1:
            raise ValueError("min_pixels must be at least 1, got %d" % min_pixels)
        max_rounds = max_objects if max_rounds is None else int(max_rounds)
        if not max_objects <= max_rounds <= L.CLUSTER_MAX_ROUNDS:
            raise ValueError("max_rounds must be in max_objects..256, got %d" % max_rounds)
        if delta_var < 0 or delta_dist < 0:
            raise ValueError("delta_var and delta_dist must not be negative")
        bandwidth = float(delta_dist if bandwidth is None else bandwidth)
        if not (bandwidth > 0.0 and bandwidth != float("inf")):
            raise ValueError("bandwidth must be positive and finite, got %r" % (bandwidth,))
        dev = self.store.device
        with torch.no_grad():
            a, _ = self._emb_act(emb)
            f = fg.to(dev)
            if f.dtype != torch.uint8:
                f = (f != 0).to(torch.uint8)
            f = f.reshape(a.n, -1).contiguous()
            assert f.shape[1] == a.h * a.w, "fg and emb differ in size"
            n_in = c0 = None
            if method == 'kmeans':
                if n_objects is None:
                    raise ValueError("method 'kmeans' needs n_objects [B]")
                n_in = n_objects.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
                assert n_in.numel() == a.n
                if not isinstance(init, str):
                    ini = init.to(device=dev, dtype=torch.float32)
                    if ini.dim() != 3 or ini.shape[0] != a.n or not 1 <= ini.shape[1] <= 32 or ini.shape[2] != a.c:
                        raise ValueError("init: 'farthest' or a tensor [B,K,C] with K <= 32, got %s" % (tuple(ini.shape),))
                    c0 = torch.zeros((a.n, 32, 32), dtype=torch.float32, device=dev)
                    c0[:, :ini.shape[1], :a.c].copy_(ini)
                    max_objects = min(max_objects, ini.shape[1])
                elif init != 'farthest':
                    raise ValueError("init: 'farthest' or a tensor [B,K,C], got %r" % (init,))
            labels, n_out, centres, sizes, moved = self.net.cluster(
                a, f, method, bandwidth=bandwidth, shifts=shifts, max_objects=max_objects, max_rounds=max_rounds,
                min_pixels=min_pixels, assign_rest=assign_rest, refine=refine, n_objects=n_in, iters=iters, init=c0)
            return dict(labels=labels.view(a.n, a.h, a.w), n_objects=n_out, centres=centres[:, :, :a.c], sizes=sizes,
                        moved=moved)

    def segment_embedding(self, x, *, sem_map=None, n_objects=None, **kw):
        """(sem_out, sem_argmax, labels, n_objects), the tuple segment() returns, with the instances taken from the
        embedding instead of the attention decoder: backbone, semantic head and the two embedding stems, then
        cluster_embedding(**kw) over the predicted foreground (or sem_map, fp32 {0,1} [B,H*W], in its place).  No decoder
        pass and no glimpse point; method='kmeans' needs n_objects [B].  Eval mode only.  The labels go into
        score_instances and clean_instances as segment's do."""
        with torch.no_grad():
            x_dec, _, B, H, W = self._backbone(x, "segment_embedding")
            net = self.net
            sem = net.sem_head(x_dec)
            self._last_sem = sem
            sem_out = net.to_nchw(sem)
            sem_argmax = net.to_nchw(net.argmax_map(sem))
            if sem_map is None:
                fg = net.class_map(sem).view(B, -1)
            else:
                fg = sem_map.to(self.store.device).reshape(B, -1)
                assert fg.shape[1] == H * W, "sem_map must be [B, H*W]"
            out = self.cluster_embedding(self.head.stems(x_dec), fg, n_objects=n_objects, **kw)
            return sem_out, sem_argmax, out["labels"], out["n_objects"]

    # ------------------------------------------------------------------ connected components, cleaning instance maps
    def _cc_map(self, maps, connectivity, min_area=1, max_objects=255):
        t = maps.to(self.store.device).contiguous()
        if t.dtype != torch.uint8 or t.dim() != 3:
            raise TypeError("expects a uint8 map [B,H,W], got %s %s" % (t.dtype, tuple(t.shape)))
        if connectivity not in (4, 8):
            raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
        if not 1 <= int(max_objects) <= 255:
            raise ValueError("max_objects must be in 1..255 (labels are uint8), got %d" % max_objects)
        if t.shape[2] % 4 or t.shape[1] * t.shape[2] >= 1 << 30 or not 1 <= t.shape[0] <= 65535:
            raise ValueError("maps [B,H,W]: W a multiple of 4, H*W < 2^30, 1 <= B <= 65535; got %s" % (tuple(t.shape),))
        return t

    def components(self, maps, *, connectivity=8):
        """(comp int32 [B,H,W], n_components int32 [B]), on the device, of a uint8 map [B,H,W] whose value 0 is background:
        two pixels belong together when they are neighbours (connectivity 4: edges, 8: edges and corners) and hold the same
        non-zero value.  comp is 0 on the background and elsewhere 1 + the smallest row-major pixel index of the pixel's
        component inside its image - the same tensor bit for bit on every run (isa_cc_label)."""
        with torch.no_grad():
            return self.net.cc_label(self._cc_map(maps, connectivity), connectivity)

    def split_components(self, maps, *, connectivity=8, min_area=1, max_objects=255):
        """(labels uint8 [B,H,W], n_objects int32 [B], dropped int32 [B]), on the device: every connected component of `maps`
        (see components()) with at least min_area pixels becomes an instance, numbered 1, 2, .. in raster order of the
        components' first pixels; past max_objects (1..255) a component gets no label and is counted in dropped.  Fed with
        class_map() or a foreground map this is the count-the-blobs baseline of a semantic-only model; the result goes
        straight into score_instances."""
        with torch.no_grad():
            t = self._cc_map(maps, connectivity, min_area, max_objects)
            comp, _ = self.net.cc_label(t, connectivity)
            return self.net.cc_select(t, comp, L.CC_SPLIT, min_area, max_objects)

    def clean_instances(self, labels, *, keep='largest', connectivity=8, min_area=1, max_objects=255):
        """Cleans a label map such as segment()'s (uint8 [B,H,W]), on the device; returns (labels, n_objects, dropped) as
        split_components does.  keep='largest': of every instance only its largest connected piece survives (equal areas:
        the one whose first pixel comes first), and only if it has min_area pixels; the survivors are renumbered 1, 2, .. in
        the order of their old labels (segment's order of discovery).  keep='all': every piece of min_area pixels becomes an
        instance of its own, in raster order.  dropped counts the pieces of min_area pixels that ended without a label."""
        if keep not in ('largest', 'all'):
            raise ValueError("keep must be 'largest' or 'all', got %r" % (keep,))
        with torch.no_grad():
            t = self._cc_map(labels, connectivity, min_area, max_objects)
            comp, _ = self.net.cc_label(t, connectivity)
            return self.net.cc_select(t, comp, L.CC_LARGEST if keep == 'largest' else L.CC_SPLIT, min_area, max_objects)

    # ------------------------------------------------------------------ measuring instances, filtering and ordering by them
    def _props_map(self, labels):
        t = labels.to(self.store.device).contiguous()
        if t.dtype != torch.uint8 or t.dim() != 3:
            raise TypeError("expects a uint8 label map [B,H,W], got %s %s" % (t.dtype, tuple(t.shape)))
        n, h, w = t.shape
        if (h * w) % 4 or max(h, w) > L.PROPS_MAX_SIDE or not 1 <= n <= 65535 or min(h, w) < 1:
            raise ValueError("labels [B,H,W]: H*W a multiple of 4, H and W at most %d, 1 <= B <= 65535; got %s"
                             % (L.PROPS_MAX_SIDE, tuple(t.shape)))
        return t

    def instance_properties(self, labels, image=None, *, n_labels=256, check=True):
        """Measurements of every instance of a uint8 label map [B,H,W] (segment's, clean_instances', ...), on the device: a
        double tensor [B, n_labels, 24] whose row v describes label v of the image and whose columns are PROPS_COLUMNS:
        area; the half-open box x0, y0, x1, y1; the centroid; the central second moments per pixel mu_xx, mu_yy, mu_xy; major
        and minor axis length 4 sqrt(lambda); eccentricity; orientation (the angle of the major axis from the x axis in
        (-pi/2, pi/2], y pointing down: the project's own convention); perimeter as crack length (pixel edges between the
        label and anything else, the image edge and holes included); touches_border; extent; equivalent diameter;
        compactness 4 pi A / P^2; the first pixel's row-major index; the mean of up to four image channels.
        x is the column, y the row.  A label that is absent (label 0 always: background is not measured) has area 0 and NaN
        elsewhere.  image: uint8 [B,H,W,C], C in 1, 3, 4 - such as the raw RGB batch forward() accepts - or None (NaN means).
        Labels >= n_labels are not measured: with check=True (one device read, the only host synchronisation) they raise
        ValueError; with check=False nothing is read back and the counts stay in self.last_props_oob (int32 [B]).
        isa_label_props + isa_instance_props; DESIGN.md section 20."""
        with torch.no_grad():
            t = self._props_map(labels)
            if not 1 <= int(n_labels) <= 256:
                raise ValueError("n_labels must be in 1..256, got %r" % (n_labels,))
            img = None
            if image is not None:
                img = image.to(self.store.device).contiguous()
                if img.dtype != torch.uint8 or img.dim() != 4 or tuple(img.shape[:3]) != tuple(t.shape) or \
                        img.shape[3] not in (1, 3, 4):
                    raise TypeError("image: uint8 %s + (C,), C in 1, 3, 4; got %s %s"
                                    % (tuple(t.shape), img.dtype, tuple(img.shape)))
            acc, oob = self.net.label_props(t, img, int(n_labels))
            out = self.net.instance_props(acc, t.shape[1], t.shape[2], 0 if img is None else img.shape[3])
            self.last_props_oob = oob
            if check:
                bad = oob.cpu()
                if int(bad.sum()):
                    raise ValueError("instance_properties: %d pixels of images %s carry a label >= n_labels = %d"
                                     % (int(bad.sum()), torch.nonzero(bad).view(-1).tolist(), int(n_labels)))
            return out

    def select_instances(self, labels, *, min_area=1, max_area=None, clear_border=False, order='label', max_objects=255):
        """Filters and renumbers the instances of a uint8 label map [B,H,W] by their measurements, on the device; returns
        (labels, n_objects, dropped) as clean_instances does, ready for score_instances.  An instance stays when it has
        min_area <= area <= max_area (None: no upper limit) pixels and, with clear_border, its box touches no image edge
        (a truncated leaf).  Those that stay are numbered 1, 2, .. by order: 'label' (the old labels ascending), 'area'
        (largest first, equal areas by the smaller old label) or 'raster' (by first pixel); past max_objects (1..255) an
        instance gets no label.  dropped counts the instances of the input that ended without one.  Nothing is read back.
        isa_label_props + isa_props_select + isa_relabel_u8."""
        orders = {'label': L.ORDER_LABEL, 'area': L.ORDER_AREA, 'raster': L.ORDER_RASTER}
        if order not in orders:
            raise ValueError("order must be 'label', 'area' or 'raster', got %r" % (order,))
        if not 1 <= int(max_objects) <= 255:
            raise ValueError("max_objects must be in 1..255 (labels are uint8), got %d" % max_objects)
        if int(min_area) < 0 or (max_area is not None and int(max_area) < 1):
            raise ValueError("min_area must not be negative and max_area must be positive or None, got %r, %r"
                             % (min_area, max_area))
        with torch.no_grad():
            t = self._props_map(labels)
            acc, _ = self.net.label_props(t, None, 256)
            table, count, dropped = self.net.props_select(acc, t.shape[1], t.shape[2], int(min_area), int(max_area or 0),
                                                          clear_border, orders[order], int(max_objects))
            return self.net.relabel(t, table), count, dropped

    # ------------------------------------------------------------------ outlines: polygons, holes, Euler number
    def _contour_map(self, labels, connectivity):
        t = labels.to(self.store.device).contiguous()
        if t.dtype != torch.uint8 or t.dim() != 3:
            raise TypeError("expects a uint8 label map [B,H,W], got %s %s" % (t.dtype, tuple(t.shape)))
        if connectivity not in (4, 8):
            raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
        n, h, w = t.shape
        if w % 4 or max(h, w) > L.CONTOUR_MAX_SIDE or not 1 <= n <= 65535 or h < 1:
            raise ValueError("labels [B,H,W]: W a multiple of 4, H and W at most %d, 1 <= B <= 65535; got %s"
                             % (L.CONTOUR_MAX_SIDE, tuple(t.shape)))
        return t

    @staticmethod
    def contour_capacities(h, w):
        """The default (max_contours, max_vertices) of contours() for an H x W map: max(256, H W / 16) contours and eight
        vertices each - 4096 and 32768 at 256 x 256, where a map of leaves has some hundred contours and a few thousand
        vertices.  The worst cases are H W contours (isolated pixels) and 4 H W vertices."""
        cmax = max(256, h * w // 16)
        return cmax, 8 * cmax

    def contours(self, labels, *, connectivity=8, max_contours=None, max_vertices=None, check=True):
        """The outlines of every instance of a uint8 label map [B,H,W], on the device: (table int64 [B,max_contours,8],
        verts int16 [B,max_vertices,2], counts int32 [B,4]).  A contour is a closed chain of pixel edges with the label on
        its right - an outer boundary (clockwise on the screen, positive area) or a hole (negative area) - and a row of
        table: label, offset of its first vertex in verts[b], vertex count, edge count (crack length), signed twice-area,
        start key, index of the pixel that owns the start edge, 0; rows in ascending order of start key.  verts holds the
        corner points (x, y) of contour 0, then of contour 1, ..: collinear points are dropped, pixel (y, x) is the square
        (x, y) .. (x+1, y+1).  connectivity 8 joins pixels of one label across a corner into one contour, 4 does not.
        counts[b]: contours found, vertices found, contours beyond max_contours, vertices beyond max_vertices; rows and
        vertices past what was found (or what fitted: the first max_contours rows, and whole contours while they fit into
        max_vertices) are uninitialised.  The capacities default to contour_capacities(H, W).  check=True reads counts (the
        call's only synchronisation) and raises ValueError on overflow; check=False reads nothing and leaves counts in
        self.last_contour_counts.  isa_contour_trace; DESIGN.md section 21."""
        with torch.no_grad():
            t = self._contour_map(labels, connectivity)
            cmax, vmax = self.contour_capacities(t.shape[1], t.shape[2])
            cmax = cmax if max_contours is None else int(max_contours)
            vmax = vmax if max_vertices is None else int(max_vertices)
            if cmax < 1 or vmax < 1:
                raise ValueError("max_contours and max_vertices must be positive, got %r, %r" % (max_contours, max_vertices))
            table, verts, counts = self.net.contour_trace(t, connectivity, cmax, vmax)
            self.last_contour_counts = counts
            if check:
                c = counts.cpu()
                if int(c[:, 2:].sum()):
                    raise ValueError("contours: images %s hold up to %d contours and %d vertices, more than max_contours = %d "
                                     "or max_vertices = %d" % (torch.nonzero(c[:, 2:].sum(1)).view(-1).tolist(),
                                                               int(c[:, 0].max()), int(c[:, 1].max()), cmax, vmax))
            return table, verts, counts

    def _contours_that_fit(self, t, connectivity, want_vertices):
        """contours() of the device map t at the default capacities and, where those overflow, once more at what was found;
        returns (table, verts, counts, counts on the host).  One read of counts per trace."""
        table, verts, counts = self.contours(t, connectivity=connectivity, check=False,
                                             max_vertices=None if want_vertices else 1)
        c = counts.cpu()
        over = c[:, 2].sum() + (c[:, 3].sum() if want_vertices else 0)
        if int(over):
            table, verts, counts = self.contours(t, connectivity=connectivity, check=False, max_contours=int(c[:, 0].max()),
                                                 max_vertices=max(1, int(c[:, 1].max())) if want_vertices else 1)
            c = counts.cpu()
        return table, verts, counts, c

    def instance_topology(self, labels, *, connectivity=8, n_labels=256):
        """int32 [B, n_labels, 3] on the device: per label of a uint8 map [B,H,W] the number of its connected components
        under `connectivity` (its outer contours), of its holes (enclosed components of everything else under the dual
        connectivity) and the Euler number, components - holes.  Label 0 and absent labels are 0.  The contour table is
        traced at the default capacity and, after one read of the counts, again at the size found if it did not fit.
        isa_contour_trace + isa_contour_topology."""
        if not 1 <= int(n_labels) <= 256:
            raise ValueError("n_labels must be in 1..256, got %r" % (n_labels,))
        with torch.no_grad():
            t = self._contour_map(labels, connectivity)
            table, _, counts, _ = self._contours_that_fit(t, connectivity, False)
            return self.net.contour_topology(table, counts, int(n_labels))

    def polygons(self, labels, *, connectivity=8):
        """The instances of a uint8 label map [B,H,W] as polygons on the host: per image a list with one entry
        {'label': int, 'outer': int16 ndarray [k,2], 'holes': [int16 ndarray [k,2], ...]} per outer contour, in table
        order; points are (x, y) corners of pixels (see contours()), the outer ring clockwise on the screen, holes
        counter-clockwise.  A hole goes to the outer contour of its own connected component (components() of the same map,
        read at the pixel that owns each contour's start edge).  Only the tables, the vertices in use and one component id
        per contour come down."""
        with torch.no_grad():
            t = self._contour_map(labels, connectivity)
            table, verts, _, counts = self._contours_that_fit(t, connectivity, True)
            comp, _ = self.components(t, connectivity=connectivity)
            n = t.shape[0]
            rows = int(counts[:, 0].max())
            ids = torch.gather(comp.view(n, -1), 1, table[:, :rows, 6].clamp(0, comp[0].numel() - 1)).cpu().numpy()
            table_h = table[:, :rows].cpu().numpy()
            verts_h = verts[:, :max(1, int(counts[:, 1].max()))].cpu().numpy()
        out = []
        for b in range(n):
            polys, by_comp = [], {}
            k = int(counts[b, 0])
            rings = [verts_h[b, int(r[1]):int(r[1] + r[2])].copy() for r in table_h[b, :k]]
            for r, ring, cid in zip(table_h[b, :k], rings, ids[b, :k]):
                if r[4] > 0:
                    polys.append({'label': int(r[0]), 'outer': ring, 'holes': []})
                    by_comp[int(cid)] = polys[-1]
            for r, ring, cid in zip(table_h[b, :k], rings, ids[b, :k]):
                if r[4] < 0:
                    by_comp[int(cid)]['holes'].append(ring)
            out.append(polys)
        return out

    # ------------------------------------------------------------------ distance transform, border weights, instance fill
    def _edt_map(self, labels):
        t = labels.to(self.store.device).contiguous()
        if t.dtype != torch.uint8 or t.dim() != 3:
            raise TypeError("expects a uint8 label map [B,H,W], got %s %s" % (t.dtype, tuple(t.shape)))
        n, h, w = t.shape
        if w % 4 or max(h, w) > L.EDT_MAX_SIDE or not 1 <= n <= 65535 or h < 1:
            raise ValueError("labels [B,H,W]: W a multiple of 4, H and W at most %d, 1 <= B <= 65535; got %s"
                             % (L.EDT_MAX_SIDE, tuple(t.shape)))
        return t

    def distance_transform(self, labels):
        """(d1sq int32, d2sq int32, nearest uint8), each [B,H,W] on the device, of a uint8 label map [B,H,W] whose value 0
        means no instance: the exact squared Euclidean distance of every pixel to the nearest instance of its image and
        to the second-nearest one (equal to d1sq where two instances tie), and the smallest label at distance d1sq.
        INT32_MAX / 0 where the image holds no instance, INT32_MAX in d2sq where it holds fewer than two.  Integers
        only: the same tensors bit for bit on every run (isa_edt2_u8)."""
        with torch.no_grad():
            return self.net.distance_transform(self._edt_map(labels))

    def border_weights(self, ins_or_labels, w0=10.0, sigma=5.0):
        """The U-Net border weight map fp32 [B,H,W] on the device: 1 on instance pixels and where the image holds fewer than
        two instances, 1 + w0 * exp(-(d1 + d2)^2 / (2 sigma^2)) on the background, d1 and d2 the distances to the two nearest
        instances.  ins_or_labels: instance planes in any form forward() takes (uint8 [B,H,W,K], int64 or fp32 [B,K,H,W]) or
        a uint8 label map [B,H,W]."""
        if float(w0) < 0 or not float(sigma) > 0:
            raise ValueError("w0 must not be negative and sigma must be positive, got %r, %r" % (w0, sigma))
        with torch.no_grad():
            t = ins_or_labels
            if t.dim() == 4:
                n = t.shape[0]
                h, w = (t.shape[1], t.shape[2]) if t.dtype == torch.uint8 else (t.shape[2], t.shape[3])
                t = self._label_map(t, "ins_or_labels")[0].view(n, h, w)
            t = self._edt_map(t)
            cfg = torch.tensor([float(w0), float(sigma)], dtype=torch.float32, device=t.device)
            return self.net.border_weights(t, cfg)

    def fill_instances(self, labels, fg, max_dist=None):
        """(labels uint8 [B,H,W], filled int32 [B]), on the device: every pixel of `labels` that is 0 while fg (uint8 or bool
        [B,H,W], non-zero = foreground, such as class_map()) is set takes the label of the nearest instance of its image,
        the smaller label on a tie (a Voronoi fill); with max_dist only when that instance lies within max_dist pixels.
        Labelled pixels and the background stay as they are; filled counts the pixels given a label."""
        if max_dist is not None and float(max_dist) < 0:
            raise ValueError("max_dist must not be negative, got %r" % (max_dist,))
        with torch.no_grad():
            t = self._edt_map(labels)
            f = fg.to(self.store.device)
            if f.dtype == torch.bool:
                f = f.to(torch.uint8)
            f = f.contiguous()
            if f.dtype != torch.uint8 or f.shape != t.shape:
                raise TypeError("fg: uint8 or bool %s, got %s %s" % (tuple(t.shape), f.dtype, tuple(f.shape)))
            bound = -1 if max_dist is None else int(min(float(max_dist) ** 2, 2 ** 31 - 1))
            return self.net.fill_labels(t, f, bound)

    # ------------------------------------------------------------------ scoring semantic predictions on the device
    def _semantic_logits(self, x):
        """Backbone and semantic head alone, eval mode: leaves the logits of `x` (either input form of forward) in
        self._last_sem for class_map() / score_semantic().  Works for instance models too (their head is not run)."""
        assert not self.training, "eval mode only (running BatchNorm statistics)"
        with torch.no_grad():
            x_dec, _ = self._eval_unet(x, "semantic")
            self._last_sem = self.net.sem_head(x_dec)

    def class_map(self):
        """uint8 class ids [B,H,W] on the device from the logits of the LAST forward() or segment(): arg-max over the
        classes, first maximum wins (isa_sem_confusion).  Must be called before the next forward (the logits live in
        that step's arena), like sem_costs."""
        sem = getattr(self, "_last_sem", None)
        assert sem is not None, "class_map() follows a forward()"
        with torch.no_grad():
            return self.net.class_map(sem)

    def score_semantic(self, sem_target, *, check=True):
        """(scores double [B, 4+2K], conf int64 [B,K,K]), both on the device, of the LAST forward's (or segment's) logits
        against sem_target: uint8 [B,H,W] class ids or one-hot int64 [B,C,H,W].  conf[b][t][p] counts the pixels of image b
        with label t and predicted class p (the arg-max, never materialised: one pass over the logits); the score columns
        are 0 pixel accuracy, 1 mean IoU and 2 mean Dice over the classes present in either map, 3 their number,
        4..4+K-1 IoU per class, 4+K..4+2K-1 Dice per class (NaN for a class absent from both maps).
        A pixel whose label is >= K is not counted; the per-image counts stay on the device in self.last_sem_oob (int32
        [B]).  With check=True (one device read, the only host synchronisation of the call) any such pixel raises
        ValueError.  Same lifetime rule as sem_costs: call it before the next forward."""
        sem = getattr(self, "_last_sem", None)
        assert sem is not None, "score_semantic() follows a forward()"
        dev, K = self.store.device, self.n_classes
        with torch.no_grad():
            t = sem_target.to(dev).contiguous()
            if t.dtype == torch.uint8:
                assert tuple(t.shape) == (sem.n, sem.h, sem.w), "compact sem_target: uint8 [B,H,W]"
                labels = t
            else:
                assert t.dtype == torch.int64 and t.dim() == 4 and tuple(t.shape[2:]) == (sem.h, sem.w) and \
                    t.shape[0] == sem.n and 2 <= t.shape[1] <= 256, "sem_target: uint8 [B,H,W] or one-hot int64 [B,C,H,W]"
                labels = self.net.labels_from_onehot(t, self._new)
            conf, oob = self.net.sem_confusion(sem, labels)
            scores = self.net.sem_scores(conf)
            self.last_sem_oob = oob
            if check:
                bad = oob.cpu()
                if int(bad.sum()):
                    raise ValueError("score_semantic: %d pixels of images %s carry a label outside the K = %d classes 0..%d"
                                     % (int(bad.sum()), torch.nonzero(bad).view(-1).tolist(), K, K - 1))
            return scores, conf

    def semantic_scores(self, conf):
        """The score rows of score_semantic for confusion matrices int64 [K,K] -> [4+2K] or [n,K,K] -> [n, 4+2K], on the
        device (isa_sem_scores) - for a total summed over images, batches or ranks."""
        with torch.no_grad():
            c = conf.to(self.store.device)
            assert c.dtype == torch.int64 and c.dim() in (2, 3) and c.shape[-1] == c.shape[-2], "int64 [K,K] or [n,K,K]"
            if not 2 <= c.shape[-1] <= 32:
                raise ValueError("2..32 classes, got %d" % c.shape[-1])
            out = self.net.sem_scores(c.reshape(-1, c.shape[-1], c.shape[-1]).contiguous())
            return out[0] if c.dim() == 2 else out

    # ------------------------------------------------------------------ forward
    def forward(self, training, *_input, selected_idx=None, injected_s_t=None, capture=None, _arena_key=None):
        """reseg.py:106-130.  (x) -> (sem_out, sem_argmax);  (x, sem_onehot[B,K,H,W] i64,
        ins[B,32,H,W] i64, N[B,1]) [or the compact uint8 pair sem[B,H,W], ins[B,H,W,32]: expanded on device] -> (sem_out, sem_argmax, ins_cost, criterion, ins_ce_loss,
        ins_dice_loss).  BatchNorm mode follows .train()/.eval() like the reference modules; the
        `training` flag drives sampling, F.dropout2d and the loss branch (attenet2.py:377-399).
        `selected_idx` / `injected_s_t` inject the reference's host RNG choices (random.shuffle,
        torch.multinomial) for parity runs; defaults: random order / argmax-or-sampled on device."""
        E, net = self.engine, self.net
        has_gt = len(_input) == 4
        if has_gt:
            x, sem_seg_target, ins_seg_target, N = _input
        else:
            x = _input[0]
        raw_rgb = x.dtype == torch.uint8           # [B,H,W,3] uint8: ImageEx runs on device (net.image_ex)
        if raw_rgb:
            assert x.dim() == 4 and x.shape[3] == 3, "uint8 input must be RGB [B,H,W,3]"
            assert x.shape[1] % 16 == 0 and x.shape[2] % 16 == 0
        else:
            assert x.dim() == 4 and x.shape[1] == 21, "expects [B,21,H,W] (ImageEx tensor, utils.py:109)"
            assert x.shape[2] % 16 == 0 and x.shape[3] % 16 == 0
        dev = self.store.device
        E.begin(bn_train=self.training, record=False,
                key=_arena_key or ("forward", has_gt, tuple(x.shape), x.dtype, bool(training)))
        if getattr(self, "_weights_dirty", True) and E.packer.entries:
            E.packer.pack()
        self._weights_dirty = False
        if has_gt and ins_seg_target.dtype == torch.uint8:      # compact targets: net.collate_targets (dataset.py:349-379)
            sem_seg_target, ins_seg_target = net.collate_targets(sem_seg_target, ins_seg_target)
        xin = net.input_view(x)
        x_dec, feats = net.unet(xin)
        if capture is not None:                    # UNet.forward's six maps (unet_model.py:36), for parity tests
            capture.update({"unet.x_dec": x_dec, "unet.x1": feats[0], "unet.x2": feats[1], "unet.x3": feats[2],
                            "unet.x4": feats[3], "unet.x5": feats[4]})
        sem = net.sem_head(x_dec)
        self._last_sem = sem                       # logits view in the step's arena (sem_costs)
        sem_out = net.to_nchw(sem)
        if has_gt:
            # (the map lives in the step's arena: the caller gets a copy)
            sem_argmax = net.onehot_map(sem_seg_target.to(dev).contiguous()).view(x.shape[0], 1, sem.h, sem.w).clone()
        else:
            sem_argmax = net.to_nchw(net.argmax_map(sem))
        if not self.use_instance_seg:
            return sem_out, sem_argmax
        if not has_gt:
            # the reference raises UnboundLocalError here (reseg.py:126): the instance head needs
            # ground-truth masks and has no GT-free mode
            raise RuntimeError("instance head needs (x, sem, ins, N); build ReSeg(.., use_instance_seg=False) "
                               "for GT-free inference")
        n_ins = [int(v) for v in N.reshape(-1).tolist()]
        if selected_idx is None:
            import random
            selected_idx = []
            for k in n_ins:                       # attenet2.py:349-355
                order = list(range(k))
                random.shuffle(order)
                selected_idx.append(order)
        sem_map = sem_argmax.reshape(x.shape[0], -1).contiguous()
        ins_dev = ins_seg_target.to(dev).contiguous()
        rec = self.head.forward(x_dec, feats, sem_map, ins_dev, n_ins, bool(training), selected_idx,
                                injected_s_t, capture)
        self.last_record = rec
        scal = rec["scal"].clone()
        ins_cost = scal[0] + float("nan") if training else scal[0]     # attenet2.py:77: H is NaN in training
        return (sem_out, sem_argmax, ins_cost, scal[1], scal[2], scal[3])
