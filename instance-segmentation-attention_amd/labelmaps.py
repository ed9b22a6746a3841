"""Device operators on label maps: scoring, connected components, measurements, outlines, distance transform, the
discriminative embedding loss and its clustering.  They take device tensors and return device
tensors and need no model: `LabelOps()` is a handle made of a device, the checked kernel library and an allocator.
`ReSeg` is a `LabelOps` (its public methods are these), and the training step owns one whose allocator is the step's
arena (`Network.maps`).  Missing library or missing GPU => hard error, never a fallback.
"""
import torch

from . import lib as L
from .engine import Act, rup

# the columns of LabelOps.instance_properties (isa_instance_props, include/isa_kernels.h)
PROPS_COLUMNS = ("area", "x0", "y0", "x1", "y1", "centroid_x", "centroid_y", "mu_xx", "mu_yy", "mu_xy", "major_axis",
                 "minor_axis", "eccentricity", "orientation", "perimeter", "touches_border", "extent", "equivalent_diameter",
                 "compactness", "first_pixel", "mean_c0", "mean_c1", "mean_c2", "mean_c3")

DISC_FORMS = {"reference": (True, (1.0, 0.0, 0.0, 0.005)), "full": (False, (1.0, 1.0, 0.001, 0.0))}


class DiscCriterion:
    """Settings of the discriminative embedding loss (DiscriminativeLoss, losses/discriminative.py:162-213) in ONE device
    buffer, allocated once and rewritten in place so that a captured hipGraph reads them at replay time.  Layout
    (include/isa_kernels.h, isa_disc_*): {delta_v, delta_d, norm, unit_means, alpha, beta, gamma, gamma_q, weight, 0, 0, 0}.
    form 'reference': what discriminative_loss() computes (unit means, var + 0.005 qreg); 'full': var + dist + 0.001 reg on
    plain means; `weights` = (alpha, beta, gamma, gamma_q) and `unit_means` override the form's.  The loss runs when
    weight > 0; on / off, the form and the norm belong to a captured step's configuration (key()), the rest does not."""

    def __init__(self, device):
        self.cfg = torch.zeros(L.DISC_CFG_FLOATS, dtype=torch.float32, device=device)
        self.set(0.0)

    def set(self, weight, delta_var=0.5, delta_dist=1.5, norm=2, form="reference", weights=None, unit_means=None):
        if form not in DISC_FORMS:
            raise ValueError("form must be one of %s, got %r" % (tuple(DISC_FORMS), form))
        if int(norm) not in (1, 2):
            raise ValueError("norm must be 1 or 2, got %r" % (norm,))
        if float(delta_var) < 0 or float(delta_dist) < 0 or float(weight) < 0:
            raise ValueError("delta_var, delta_dist and the weight must not be negative")
        unit, w = DISC_FORMS[form]
        if weights is not None:
            w = tuple(float(v) for v in weights)
            if len(w) != 4:
                raise ValueError("weights: (alpha, beta, gamma, gamma_q)")
        if unit_means is not None:
            unit = bool(unit_means)
        self.weight, self.norm, self.form, self.on = float(weight), int(norm), form, float(weight) > 0
        self.cfg.copy_(torch.tensor([float(delta_var), float(delta_dist), float(norm), float(unit)] + list(w) +
                                    [float(weight), 0.0, 0.0, 0.0]))

    def set_weight(self, weight):
        """In place: a captured step follows it (on / off is part of the step's configuration and stays)."""
        assert float(weight) > 0 and self.on, "the weight of a running loss; switch it on or off with set()"
        self.weight = float(weight)
        self.cfg[8:9].fill_(float(weight))

    def key(self):
        return (True, self.form, self.norm) if self.on else (False, None, None)


class LabelOps:
    """The label-map operators behind one handle.  device: where they run (default: the current CUDA device, looked up
    when the first operator runs, so that a handle can be built without a GPU); lib: the kernel library (default
    L.checked(); the engine passes its profiled one); alloc(shape, dtype): where every output and every scratch buffer
    comes from (default: new tensors on `device`).
    Launches go to the current stream (L.stream_ptr()).  Two layers: launch-level methods (contiguous device tensors
    in, preconditions as asserts, allocation, launch) and the public methods on top, which convert and validate."""

    n_classes = 2          # what score_instances takes a compact sem_target to hold; a model sets its own

    def __init__(self, device=None, lib=None, alloc=None):
        self._device = None if device is None else torch.device(device)
        self.lib, self._alloc = lib or L.checked(), alloc

    @property
    def device(self):
        if self._device is None or self._device.index is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    def alloc(self, shape, dtype):
        return self._alloc(shape, dtype) if self._alloc else torch.empty(shape, dtype=dtype, device=self.device)

    # ------------------------------------------------------------------ arguments
    def _map(self, maps, quad, side=None, pixels=None, connectivity=None, max_objects=None):
        """The uint8 map [B,H,W] `maps` on the device, contiguous, after the checks every operator shares: `quad` ('W' or
        'H*W') a multiple of 4, H and W at most `side`, H*W below `pixels`, connectivity 4 or 8, max_objects in 1..255 -
        each where given."""
        t = maps.to(self.device).contiguous()
        if t.dtype != torch.uint8 or t.dim() != 3:
            raise TypeError("expects a uint8 label map [B,H,W], got %s %s" % (t.dtype, tuple(t.shape)))
        if connectivity is not None and connectivity not in (4, 8):
            raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
        if max_objects is not None and not 1 <= int(max_objects) <= 255:
            raise ValueError("max_objects must be in 1..255 (labels are uint8), got %d" % max_objects)
        n, h, w = t.shape
        ok = (w if quad == 'W' else h * w) % 4 == 0 and 1 <= n <= 65535 and min(h, w) >= 1
        limits = "%s a multiple of 4" % quad
        if side is not None:
            ok, limits = ok and max(h, w) <= side, limits + ", H and W at most %d" % side
        if pixels is not None:
            ok, limits = ok and h * w < pixels, limits + ", H*W < 2^%d" % (pixels.bit_length() - 1)
        if not ok:
            raise ValueError("labels [B,H,W]: %s, 1 <= B <= 65535; got %s" % (limits, tuple(t.shape)))
        return t

    @staticmethod
    def _refuse(counts, text):
        """Reads the per-image counts [B] or [B,k] (the one device read of a check=True call; none for counts that are on
        the host already) and raises ValueError(text % (their sum, the images that have one)) unless all are zero."""
        bad = counts.cpu()
        if int(bad.sum()):
            raise ValueError(text % (int(bad.sum()), torch.nonzero(bad.reshape(bad.shape[0], -1).sum(1)).view(-1).tolist()))

    def _label_map(self, planes, what):
        """uint8 label map [B, H*W] of ground-truth planes in either form forward() takes (isa_labels_from_planes)."""
        t = planes.to(self.device).contiguous()
        assert t.dim() == 4, "%s must be uint8 [B,H,W,K] or int64 [B,K,H,W]" % what
        out, k = self.labels_from_planes(t, what)
        return out.view(out.shape[0], -1), k

    def _emb_act(self, emb):
        """(Act, emb was one already) of an embedding: an engine Act as it is, fp32 or bf16 [B,C,H,W] copied into NHWC."""
        as_act = isinstance(emb, Act)
        if as_act:
            a = emb
        else:
            dev = self.device
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

    # ------------------------------------------------------------------ launch level: allocate through self.alloc, launch
    def labels_from_planes(self, planes: torch.Tensor, what):
        """(uint8 label map [n,h,w], k) of k instance planes in any form forward() takes: uint8 [n,h,w,k], int64 or fp32
        [n,k,h,w]; 0 = background, i + 1 = plane i, the first plane gets an overlap (isa_labels_from_planes).
        what: the argument's name in the error text."""
        form = {torch.uint8: L.PLANES_U8_NHWK, torch.int64: L.PLANES_I64_NKHW,
                torch.float32: L.PLANES_F32_NKHW}.get(planes.dtype)
        if form is None:
            raise TypeError("%s: uint8 [B,H,W,K], int64 [B,K,H,W] or fp32 [B,K,H,W], got %s" % (what, planes.dtype))
        n, h, w, k = planes.shape if form == L.PLANES_U8_NHWK else (planes.shape[i] for i in (0, 2, 3, 1))
        assert planes.is_contiguous(), "%s must be contiguous" % what
        lab = self.alloc((n, h, w), torch.uint8)
        self.lib.isa_labels_from_planes(planes, form, n, k, h * w, lab, L.stream_ptr())
        return lab, k

    def labels_from_onehot(self, onehot: torch.Tensor):
        """uint8 label map [n,h,w] of a one-hot int64 [n,K,h,w] (isa_labels_from_onehot)."""
        n, K, h, w = onehot.shape
        labels = self.alloc((n, h, w), torch.uint8)
        self.lib.isa_labels_from_onehot(onehot, n, K, h * w, labels, None, L.stream_ptr())
        return labels

    def pair_scores(self, a, b, na, nb, n_a, n_b, oob):
        """[B,8] scores (isa_instance_scores) of the uint8 maps a, b [B, L]; the out-of-range counts go to oob [B]."""
        n, Lp = a.shape
        if not (1 <= na <= 256 and 1 <= nb <= 256 and na * nb <= 16384):
            raise ValueError("label ids: %d x %d counters; each side at most 256 and the product at most 16384" % (na, nb))
        hist, out = self.alloc((n, na, nb), torch.int32), self.alloc((n, 8), torch.float64)
        self.lib.isa_label_pair_hist(a, b, n, Lp, na, nb, hist, oob, L.HIST_AGGREGATE, L.stream_ptr())
        self.lib.isa_instance_scores(hist, n, na, nb, n_a, n_b, out, L.stream_ptr())
        return out

    def sem_scores(self, conf: torch.Tensor) -> torch.Tensor:
        """double [n, 4+2K] from confusion matrices int64 [n,K,K] (isa_sem_scores): pixel accuracy, mean IoU, mean Dice,
        classes present, IoU[K], Dice[K]."""
        n, K = conf.shape[0], conf.shape[1]
        out = self.alloc((n, 4 + 2 * K), torch.float64)
        self.lib.isa_sem_scores(conf, n, K, out, L.stream_ptr())
        return out

    def cc_label(self, maps: torch.Tensor, connectivity=8):
        """(comp int32 [n,h,w], n_comp int32 [n]) of the uint8 map [n,h,w] on the device (isa_cc_label): 0 for background,
        else 1 + the smallest row-major pixel index of the pixel's component inside its image."""
        assert maps.dtype == torch.uint8 and maps.dim() == 3 and maps.is_contiguous(), "maps: contiguous uint8 [n,h,w]"
        n, h, w = maps.shape
        comp, n_comp = self.alloc((n, h, w), torch.int32), self.alloc((n,), torch.int32)
        scratch = self.alloc((L.cc_label_scratch_bytes(n, h, w),), torch.uint8)
        self.lib.isa_cc_label(maps, n, h, w, int(connectivity), comp, n_comp, scratch, scratch.numel(), L.stream_ptr())
        return comp, n_comp

    def cc_select(self, maps: torch.Tensor, comp: torch.Tensor, mode, min_area=1, max_objects=255):
        """(labels uint8 [n,h,w], count int32 [n], dropped int32 [n]) from a uint8 map and its cc_label components
        (isa_cc_select), mode L.CC_SPLIT or L.CC_LARGEST."""
        assert maps.dtype == torch.uint8 and maps.dim() == 3 and maps.is_contiguous(), "maps: contiguous uint8 [n,h,w]"
        assert comp.dtype == torch.int32 and comp.shape == maps.shape and comp.is_contiguous()
        n, h, w = maps.shape
        out = self.alloc((n, h, w), torch.uint8)
        count, dropped = self.alloc((n,), torch.int32), self.alloc((n,), torch.int32)
        scratch = self.alloc((L.cc_select_scratch_bytes(n, h, w),), torch.uint8)
        self.lib.isa_cc_select(maps, comp, n, h, w, int(mode), int(min_area), int(max_objects), out, count, dropped, scratch,
                               scratch.numel(), L.stream_ptr())
        return out, count, dropped

    def label_props(self, labels: torch.Tensor, image: torch.Tensor = None, n_labels=256):
        """(acc int64 [n,n_labels,16], oob int32 [n]) of a uint8 label map [n,h,w] and an optional uint8 image [n,h,w,c]
        (isa_label_props): area, box, raw moments, crack perimeter, first pixel and channel sums per label."""
        assert labels.dtype == torch.uint8 and labels.dim() == 3 and labels.is_contiguous(), "labels: contiguous uint8 [n,h,w]"
        n, h, w = labels.shape
        c = 0
        if image is not None:
            assert image.dtype == torch.uint8 and image.dim() == 4 and image.is_contiguous() and \
                tuple(image.shape[:3]) == (n, h, w), "image: contiguous uint8 [n,h,w,c]"
            c = image.shape[3]
        acc, oob = self.alloc((n, n_labels, L.PROPS_ACC), torch.int64), self.alloc((n,), torch.int32)
        self.lib.isa_label_props(labels, image, n, h, w, c, int(n_labels), acc, oob, L.stream_ptr())
        return acc, oob

    def instance_props(self, acc: torch.Tensor, h, w, c=0) -> torch.Tensor:
        """double [n,n_labels,24] of label_props' accumulators (isa_instance_props)."""
        n, nl = acc.shape[0], acc.shape[1]
        out = self.alloc((n, nl, L.PROPS_OUT), torch.float64)
        self.lib.isa_instance_props(acc, n, nl, int(h), int(w), int(c), out, L.stream_ptr())
        return out

    def props_select(self, acc: torch.Tensor, h, w, min_area=1, max_area=0, clear_border=False, order=L.ORDER_LABEL,
                     max_objects=255):
        """(table uint8 [n,256], count int32 [n], dropped int32 [n]) from label_props' accumulators (isa_props_select):
        the new label of every old one after filtering by area and border contact and ranking by `order`."""
        n, nl = acc.shape[0], acc.shape[1]
        table = self.alloc((n, 256), torch.uint8)
        count, dropped = self.alloc((n,), torch.int32), self.alloc((n,), torch.int32)
        self.lib.isa_props_select(acc, n, nl, int(h), int(w), int(min_area), int(max_area), int(bool(clear_border)),
                                  int(order), int(max_objects), table, count, dropped, L.stream_ptr())
        return table, count, dropped

    def relabel(self, labels: torch.Tensor, table: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """table[i][labels[i]] of a uint8 map [n,...] (isa_relabel_u8); out may be labels itself (default: allocated)."""
        assert labels.dtype == torch.uint8 and labels.is_contiguous() and table.dtype == torch.uint8 and table.is_contiguous()
        n = labels.shape[0]
        assert tuple(table.shape) == (n, 256)
        out = self.alloc(tuple(labels.shape), torch.uint8) if out is None else out
        self.lib.isa_relabel_u8(labels, table, n, labels.numel() // n, out, L.stream_ptr())
        return out

    def contour_trace(self, labels: torch.Tensor, connectivity, cmax, vmax):
        """(table int64 [n,cmax,8], verts int16 [n,vmax,2], counts int32 [n,4]) of a uint8 label map [n,h,w]
        (isa_contour_trace): every contour in ascending order of start key, its corner points, and what was found against
        what fitted.  Rows and vertices past the counts are uninitialised."""
        assert labels.dtype == torch.uint8 and labels.dim() == 3 and labels.is_contiguous(), "labels: contiguous uint8 [n,h,w]"
        n, h, w = labels.shape
        table, verts = self.alloc((n, int(cmax), L.CONTOUR_COLS), torch.int64), self.alloc((n, int(vmax), 2), torch.int16)
        counts = self.alloc((n, 4), torch.int32)
        scratch = self.alloc((L.contour_scratch_bytes(n, h, w),), torch.uint8)
        self.lib.isa_contour_trace(labels, n, h, w, int(connectivity), int(cmax), int(vmax), table, verts, counts, scratch,
                                   scratch.numel(), L.stream_ptr())
        return table, verts, counts

    def contour_topology(self, table: torch.Tensor, counts: torch.Tensor, n_labels=256) -> torch.Tensor:
        """int32 [n,n_labels,3] from contour_trace's table and counts (isa_contour_topology): outer contours, holes and
        Euler number per label."""
        n, cmax = table.shape[0], table.shape[1]
        topo = self.alloc((n, int(n_labels), 3), torch.int32)
        self.lib.isa_contour_topology(table, counts, n, cmax, int(n_labels), topo, L.stream_ptr())
        return topo

    def edt2(self, labels: torch.Tensor, want=(True, True, True)):
        """(d1sq int32, d2sq int32, nearest uint8), each [n,h,w] or None where `want` says so, of the uint8 label map
        [n,h,w] on the device (isa_edt2_u8)."""
        assert labels.dtype == torch.uint8 and labels.dim() == 3 and labels.is_contiguous(), "labels: contiguous uint8 [n,h,w]"
        n, h, w = labels.shape
        d1 = self.alloc((n, h, w), torch.int32) if want[0] else None
        d2 = self.alloc((n, h, w), torch.int32) if want[1] else None
        near = self.alloc((n, h, w), torch.uint8) if want[2] else None
        scratch = self.alloc((L.edt_scratch_bytes(n, h, w),), torch.uint8)
        self.lib.isa_edt2_u8(labels, n, h, w, d1, d2, near, scratch, scratch.numel(), L.stream_ptr())
        return d1, d2, near

    def border_map(self, labels: torch.Tensor, cfg: torch.Tensor):
        """fp32 [n,h,w] border weight map of the uint8 instance label map [n,h,w] (isa_edt2_u8 + isa_border_weights);
        cfg: device float[2] = {w0, sigma}, read by the kernel at run time."""
        n, h, w = labels.shape
        d1, d2, _ = self.edt2(labels, (True, True, False))
        out = self.alloc((n, h, w), torch.float32)
        self.lib.isa_border_weights(labels, d1, d2, cfg, n, h * w, out, L.stream_ptr())
        return out

    def fill_labels(self, labels: torch.Tensor, fg: torch.Tensor, max_dist_sq=-1):
        """(labels uint8 [n,h,w], filled int32 [n]): every pixel with label 0 and fg != 0 takes the nearest label when
        that lies within max_dist_sq (< 0: no limit) (isa_edt2_u8 + isa_fill_labels)."""
        n, h, w = labels.shape
        assert fg.dtype == torch.uint8 and fg.shape == labels.shape and fg.is_contiguous(), "fg: contiguous uint8 [n,h,w]"
        d1, _, near = self.edt2(labels, (True, False, True))
        out, filled = self.alloc((n, h, w), torch.uint8), self.alloc((n,), torch.int32)
        self.lib.isa_fill_labels(labels, fg, near, d1, int(max_dist_sq), n, h * w, out, filled, L.stream_ptr())
        return out, filled

    def disc_loss(self, emb: Act, labels: torch.Tensor, k, n_obj: torch.Tensor, cfg: torch.Tensor, norm):
        """The forward launches of the discriminative embedding loss on `emb` (isa_disc_sums, _means, _hinge, _assemble):
        labels uint8 [n, h*w] of k planes, n_obj int32 [n], cfg the settings buffer.  Returns (scal [8] = {loss, var, dist,
        reg, qreg, present instances, their pixels, 0}, mu [n,32,32], grad) where grad(demb: Act, accumulate) launches
        isa_disc_grad."""
        lib, alloc = self.lib, self.alloc
        n, hw = emb.n, emb.h * emb.w
        ch = L.disc_chunks(hw)
        f32, i32 = torch.float32, torch.int32
        slab, hslab = alloc((n * ch * 1024,), f32), alloc((n * ch * 1024,), f32)
        cslab = alloc((n * ch * 32,), i32)
        mu, m, gconst = alloc((n, 32, 32), f32), alloc((n, 32, 32), f32), alloc((n, 32, 32), f32)
        mnorm, cnt = alloc((n * 32,), f32), alloc((n * L.DISC_CNT_STRIDE,), i32)
        partial, img = alloc((n * ch * 2,), torch.float64), alloc((n * 8,), torch.float64)
        coef, scal = alloc((n + 1,), f32), alloc((8,), f32)
        lib.isa_disc_sums(emb.d(), labels, k, slab, cslab, L.stream_ptr())
        lib.isa_disc_means(slab, cslab, n_obj, cfg, n, hw, mu, m, mnorm, cnt, L.stream_ptr())
        lib.isa_disc_hinge(emb.d(), labels, k, n_obj, mu, cfg, norm, hslab, partial, L.stream_ptr())
        lib.isa_disc_assemble(hslab, partial, mu, mnorm, cnt, n_obj, cfg, norm, n, hw, gconst, coef, img, scal,
                              L.stream_ptr())

        def grad(demb: Act, accumulate):
            lib.isa_disc_grad(emb.d(), labels, k, n_obj, mu, gconst, coef, cfg, norm, demb.d(), int(accumulate),
                              L.stream_ptr())
        return scal, mu, grad

    def cluster(self, emb: Act, fg: torch.Tensor, method, *, bandwidth=1.5, shifts=3, max_objects=32, max_rounds=None,
                min_pixels=1, assign_rest=True, refine=0, n_objects=None, iters=10, init=None):
        """Clusters the embedding `emb` over the foreground fg (uint8 [n, h*w], non-zero = foreground) per image:
        isa_cluster_meanshift, or isa_cluster_kmeans from the counts n_objects (int32 [n]) and init (None: farthest-point, or
        float [n,32,32]).  max_rounds (default max_objects): the mean-shift's round budget, refused balls included.
        refine > 0 runs that many Lloyd iterations from the mean-shift's centres over the whole foreground.  Returns (labels uint8 [n, h*w], n_objects int32 [n], centres float [n,32,32], sizes int32 [n,32], moved
        int32 [n]); everything stays on the device and nothing is read back."""
        lib, alloc = self.lib, self.alloc
        n, hw = emb.n, emb.h * emb.w
        labels = alloc((n, hw), torch.uint8)
        n_out, moved = alloc((n,), torch.int32), alloc((n,), torch.int32)
        centres, sizes = alloc((n, 32, 32), torch.float32), alloc((n, 32), torch.int32)
        scratch = alloc((L.cluster_scratch_bytes(n, hw),), torch.uint8)
        outs = (labels, n_out, centres, sizes, moved, scratch, L.stream_ptr())
        if method == 'meanshift':
            rounds = int(max_objects if max_rounds is None else max_rounds)
            lib.isa_cluster_meanshift(emb.d(), fg, float(bandwidth), int(shifts), int(max_objects), rounds,
                                      int(min_pixels), int(bool(assign_rest)), *outs)
            if refine > 0:
                n_in, init = alloc((n,), torch.int32).copy_(n_out), alloc((n, 32, 32), torch.float32).copy_(centres)
                lib.isa_cluster_kmeans(emb.d(), fg, n_in, init, 32, int(refine), *outs)
        else:
            lib.isa_cluster_kmeans(emb.d(), fg, n_objects, init, int(max_objects), int(iters), *outs)
        return labels, n_out, centres, sizes, moved

    # ------------------------------------------------------------------ scoring instance predictions on the device
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
        dev = self.device
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
            oob = self.alloc((2, B), torch.int32)
            out = self.pair_scores(gt, pred, k + 1, int(max_objects) + 1, n_gt, n_pred, oob[0])
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
                    fg_gt = self.labels_from_onehot(st).view(st.shape[0], -1)
                assert tuple(fg_gt.shape) == tuple(pred.shape) == tuple(fg_pred.shape)
                sem = self.pair_scores(fg_gt, fg_pred, nc, 2, None, None, oob[1])
                out[:, 6].copy_(sem[:, 6])
                limits.append("semantic classes 0..%d" % (nc - 1))
            else:
                oob[1].zero_()
            self.last_score_oob = oob                     # for callers that pass check=False and read it with their own copy
            if check:
                for row, limit in zip(oob.cpu(), limits):
                    self._refuse(row, "score_instances: %%d pixels of images %%s carry a label outside the histogram (%s); "
                                      "at most 256 ids a side and 16384 pairs are counted" % limit)
            return out

    def semantic_scores(self, conf):
        """The score rows of score_semantic for confusion matrices int64 [K,K] -> [4+2K] or [n,K,K] -> [n, 4+2K], on the
        device (isa_sem_scores) - for a total summed over images, batches or ranks."""
        with torch.no_grad():
            c = conf.to(self.device)
            assert c.dtype == torch.int64 and c.dim() in (2, 3) and c.shape[-1] == c.shape[-2], "int64 [K,K] or [n,K,K]"
            if not 2 <= c.shape[-1] <= 32:
                raise ValueError("2..32 classes, got %d" % c.shape[-1])
            out = self.sem_scores(c.reshape(-1, c.shape[-1], c.shape[-1]).contiguous())
            return out[0] if c.dim() == 2 else out

    # ------------------------------------------------------------------ discriminative embedding loss
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
        dev = self.device
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
            scal, mu, gfn = self.disc_loss(a, labels, k, n_obj, crit.cfg, crit.norm)
            out = dict(loss=scal[0], var=scal[1], dist=scal[2], reg=scal[3], qreg=scal[4], means=mu[:, :k, :a.c])
            if grad:
                g = Act(self.alloc(tuple(a.buf.shape), a.buf.dtype), a.c0, a.c)
                gfn(g, 0)
                out["grad"] = g if as_act else g.buf[..., :a.c].permute(0, 3, 1, 2)
            return out

    # ------------------------------------------------------------------ clustering the instance embedding into instances
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
        dev = self.device
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
            labels, n_out, centres, sizes, moved = self.cluster(
                a, f, method, bandwidth=bandwidth, shifts=shifts, max_objects=max_objects, max_rounds=max_rounds,
                min_pixels=min_pixels, assign_rest=assign_rest, refine=refine, n_objects=n_in, iters=iters, init=c0)
            return dict(labels=labels.view(a.n, a.h, a.w), n_objects=n_out, centres=centres[:, :, :a.c], sizes=sizes,
                        moved=moved)

    # ------------------------------------------------------------------ connected components, cleaning instance maps
    def components(self, maps, *, connectivity=8):
        """(comp int32 [B,H,W], n_components int32 [B]), on the device, of a uint8 map [B,H,W] whose value 0 is background:
        two pixels belong together when they are neighbours (connectivity 4: edges, 8: edges and corners) and hold the same
        non-zero value.  comp is 0 on the background and elsewhere 1 + the smallest row-major pixel index of the pixel's
        component inside its image - the same tensor bit for bit on every run (isa_cc_label)."""
        with torch.no_grad():
            return self.cc_label(self._map(maps, 'W', pixels=1 << 30, connectivity=connectivity), connectivity)

    def split_components(self, maps, *, connectivity=8, min_area=1, max_objects=255):
        """(labels uint8 [B,H,W], n_objects int32 [B], dropped int32 [B]), on the device: every connected component of `maps`
        (see components()) with at least min_area pixels becomes an instance, numbered 1, 2, .. in raster order of the
        components' first pixels; past max_objects (1..255) a component gets no label and is counted in dropped.  Fed with
        class_map() or a foreground map this is the count-the-blobs baseline of a semantic-only model; the result goes
        straight into score_instances."""
        with torch.no_grad():
            t = self._map(maps, 'W', pixels=1 << 30, connectivity=connectivity, max_objects=max_objects)
            comp, _ = self.cc_label(t, connectivity)
            return self.cc_select(t, comp, L.CC_SPLIT, min_area, max_objects)

    def clean_instances(self, labels, *, keep='largest', connectivity=8, min_area=1, max_objects=255):
        """Cleans a label map such as segment()'s (uint8 [B,H,W]), on the device; returns (labels, n_objects, dropped) as
        split_components does.  keep='largest': of every instance only its largest connected piece survives (equal areas:
        the one whose first pixel comes first), and only if it has min_area pixels; the survivors are renumbered 1, 2, .. in
        the order of their old labels (segment's order of discovery).  keep='all': every piece of min_area pixels becomes an
        instance of its own, in raster order.  dropped counts the pieces of min_area pixels that ended without a label."""
        if keep not in ('largest', 'all'):
            raise ValueError("keep must be 'largest' or 'all', got %r" % (keep,))
        with torch.no_grad():
            t = self._map(labels, 'W', pixels=1 << 30, connectivity=connectivity, max_objects=max_objects)
            comp, _ = self.cc_label(t, connectivity)
            return self.cc_select(t, comp, L.CC_LARGEST if keep == 'largest' else L.CC_SPLIT, min_area, max_objects)

    # ------------------------------------------------------------------ measuring instances, filtering and ordering by them
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
            t = self._map(labels, 'H*W', side=L.PROPS_MAX_SIDE)
            if not 1 <= int(n_labels) <= 256:
                raise ValueError("n_labels must be in 1..256, got %r" % (n_labels,))
            img = None
            if image is not None:
                img = image.to(self.device).contiguous()
                if img.dtype != torch.uint8 or img.dim() != 4 or tuple(img.shape[:3]) != tuple(t.shape) or \
                        img.shape[3] not in (1, 3, 4):
                    raise TypeError("image: uint8 %s + (C,), C in 1, 3, 4; got %s %s"
                                    % (tuple(t.shape), img.dtype, tuple(img.shape)))
            acc, oob = self.label_props(t, img, int(n_labels))
            out = self.instance_props(acc, t.shape[1], t.shape[2], 0 if img is None else img.shape[3])
            self.last_props_oob = oob
            if check:
                self._refuse(oob, "instance_properties: %%d pixels of images %%s carry a label >= n_labels = %d"
                                  % int(n_labels))
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
            t = self._map(labels, 'H*W', side=L.PROPS_MAX_SIDE)
            acc, _ = self.label_props(t, None, 256)
            table, count, dropped = self.props_select(acc, t.shape[1], t.shape[2], int(min_area), int(max_area or 0),
                                                      clear_border, orders[order], int(max_objects))
            return self.relabel(t, table), count, dropped

    # ------------------------------------------------------------------ outlines: polygons, holes, Euler number
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
            t = self._map(labels, 'W', side=L.CONTOUR_MAX_SIDE, connectivity=connectivity)
            cmax, vmax = self.contour_capacities(t.shape[1], t.shape[2])
            cmax = cmax if max_contours is None else int(max_contours)
            vmax = vmax if max_vertices is None else int(max_vertices)
            if cmax < 1 or vmax < 1:
                raise ValueError("max_contours and max_vertices must be positive, got %r, %r" % (max_contours, max_vertices))
            table, verts, counts = self.contour_trace(t, connectivity, cmax, vmax)
            self.last_contour_counts = counts
            if check:
                c = counts.cpu()
                self._refuse(c[:, 2:], "contours: %%d contours and vertices of images %%s do not fit max_contours = %d and "
                                       "max_vertices = %d; an image holds up to %d contours and %d vertices"
                                       % (cmax, vmax, int(c[:, 0].max()), int(c[:, 1].max())))
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
            t = self._map(labels, 'W', side=L.CONTOUR_MAX_SIDE, connectivity=connectivity)
            table, _, counts, _ = self._contours_that_fit(t, connectivity, False)
            return self.contour_topology(table, counts, int(n_labels))

    def polygons(self, labels, *, connectivity=8):
        """The instances of a uint8 label map [B,H,W] as polygons on the host: per image a list with one entry
        {'label': int, 'outer': int16 ndarray [k,2], 'holes': [int16 ndarray [k,2], ...]} per outer contour, in table
        order; points are (x, y) corners of pixels (see contours()), the outer ring clockwise on the screen, holes
        counter-clockwise.  A hole goes to the outer contour of its own connected component (components() of the same map,
        read at the pixel that owns each contour's start edge).  Only the tables, the vertices in use and one component id
        per contour come down."""
        with torch.no_grad():
            t = self._map(labels, 'W', side=L.CONTOUR_MAX_SIDE, connectivity=connectivity)
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
    def distance_transform(self, labels):
        """(d1sq int32, d2sq int32, nearest uint8), each [B,H,W] on the device, of a uint8 label map [B,H,W] whose value 0
        means no instance: the exact squared Euclidean distance of every pixel to the nearest instance of its image and
        to the second-nearest one (equal to d1sq where two instances tie), and the smallest label at distance d1sq.
        INT32_MAX / 0 where the image holds no instance, INT32_MAX in d2sq where it holds fewer than two.  Integers
        only: the same tensors bit for bit on every run (isa_edt2_u8)."""
        with torch.no_grad():
            return self.edt2(self._map(labels, 'W', side=L.EDT_MAX_SIDE))

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
            t = self._map(t, 'W', side=L.EDT_MAX_SIDE)
            cfg = torch.tensor([float(w0), float(sigma)], dtype=torch.float32, device=t.device)
            return self.border_map(t, cfg)

    def fill_instances(self, labels, fg, max_dist=None):
        """(labels uint8 [B,H,W], filled int32 [B]), on the device: every pixel of `labels` that is 0 while fg (uint8 or bool
        [B,H,W], non-zero = foreground, such as class_map()) is set takes the label of the nearest instance of its image,
        the smaller label on a tie (a Voronoi fill); with max_dist only when that instance lies within max_dist pixels.
        Labelled pixels and the background stay as they are; filled counts the pixels given a label."""
        if max_dist is not None and float(max_dist) < 0:
            raise ValueError("max_dist must not be negative, got %r" % (max_dist,))
        with torch.no_grad():
            t = self._map(labels, 'W', side=L.EDT_MAX_SIDE)
            f = fg.to(self.device)
            if f.dtype == torch.bool:
                f = f.to(torch.uint8)
            f = f.contiguous()
            if f.dtype != torch.uint8 or f.shape != t.shape:
                raise TypeError("fg: uint8 or bool %s, got %s %s" % (tuple(t.shape), f.dtype, tuple(f.shape)))
            bound = -1 if max_dist is None else int(min(float(max_dist) ** 2, 2 ** 31 - 1))
            return self.fill_labels(t, f, bound)
