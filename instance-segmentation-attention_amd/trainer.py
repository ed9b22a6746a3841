"""Training step on the HIP engine (reference: code/lib/model.py:190-284 `__minibatch`, :145-166 optimizer).

One step = zero the flat gradient buffer, forward with the backward tape recorded (semantic CE + Dice,
attention-head losses assembled on device), hand-written backward, one RCCL all-reduce of the flat
gradient buffer when world_size > 1, global-norm clip (10) + Adadelta(lr=1,
weight_decay=1e-3) fused in one kernel over the trainable slice.  No host sync inside the step.
optimizer= selects Adam, RMSprop or SGD instead (csrc/optim.hip: the same fused clip + decay + update); train_cnn=False
freezes the backbone: norm, all-reduce and update cover the trainable slice behind the `base.*` prefix only.
"""
import random

import torch

from . import lib as L
from .parallel import exchange_and_update


OPTIMIZERS = ('Adadelta', 'Adam', 'RMSprop', 'SGD')                         # model.py:147


def frozen_prefix(store):
    """Floats of the `base.*` parameters, which open the schema and therefore the trainable slice: [0, n_base)."""
    base = [n for n in store.names if n.startswith("base.") and n not in store.int_buffers
            and store.offsets[n] < store.n_train]
    n_base = sum((store.numel(n) + 3) // 4 * 4 for n in base)
    rest = [store.offsets[n] for n in store.names if n not in store.int_buffers and not n.startswith("base.")]
    assert base and max(store.offsets[n] for n in base) < n_base <= min(rest) and n_base % 4 == 0, \
        "base.* is not a contiguous prefix of the trainable slice"
    return n_base


class Trainer:
    def __init__(self, model, world_size=1, lr=1.0, weight_decay=1e-3, clip_grad_norm=10.0, rho=0.9, eps=1e-6,
                 criterion='Multi', class_weights=None, optimize_bg=False, optimizer='Adadelta', train_cnn=True,
                 lovasz_per_image=False, lovasz_only_present=False, disc_weight=0.0, delta_var=0.5, delta_dist=1.5,
                 disc_norm=2, disc_form='reference', border_weight=0.0, border_sigma=5.0):
        assert optimizer in OPTIMIZERS, optimizer
        self.model = model
        self.optimizer, self.train_cnn = optimizer, bool(train_cnn)
        # semantic criterion (model.py:102-133, 255-269): written once into the model's settings buffer, which was
        # allocated with the model - a captured step keeps reading the same device memory
        # off first: an earlier Trainer's border term must not refuse this one's criterion.  (This resets a border term set
        # directly on model.net.crit as well: like the criterion, the term is the Trainer's to set.)
        model.net.crit.set_border(0.0)
        model.set_criterion(criterion, class_weights, optimize_bg, lovasz_per_image, lovasz_only_present)
        self.criterion = criterion
        # the border term: the CE of every pixel weighted by the U-Net border map of the step's
        # instance targets, computed on the device inside the step; 0 = off, and then nothing of it runs
        model.net.crit.set_border(border_weight, border_sigma)
        # the discriminative loss on the instance embedding (DiscriminativeLoss(delta_var, delta_dist, norm), model.py:109-115):
        # runs when disc_weight > 0 and the model has an instance head; its settings live in a device buffer of the model
        model.net.disc.set(disc_weight, delta_var, delta_dist, disc_norm, disc_form)
        self.world = world_size
        self.lr, self.wd, self.clip, self.rho, self.eps = lr, weight_decay, clip_grad_norm, rho, eps
        st = model.store
        # the updated range [lo, n_train) of the flat buffers.  train_cnn=False (model.py:196-202: requires_grad=False on
        # model.base): the backbone has no gradient there, so clip_grad_norm_ and the optimizer skip it, decay included
        self.lo = 0 if self.train_cnn else frozen_prefix(st)
        n = st.n_train - self.lo
        zeros = lambda: torch.zeros(n, dtype=torch.float32, device=st.device)
        # torch.optim's state names; library defaults for what the reference does not set (model.py:150-162)
        if optimizer == 'Adadelta':
            self.state = dict(square_avg=zeros(), acc_delta=zeros())
            self.sq, self.acc = self.state["square_avg"], self.state["acc_delta"]
        elif optimizer == 'Adam':
            self.betas, self.adam_eps = (0.9, 0.999), 1e-8
            # step: the update count, advanced on the device so that a replayed graph keeps its bias correction exact;
            # aux: the scalars isa_adam's first launch hands its second
            self.state = dict(exp_avg=zeros(), exp_avg_sq=zeros(), step=torch.zeros(1, dtype=torch.int32, device=st.device))
            self._adam_aux = torch.zeros(4, dtype=torch.float32, device=st.device)
        elif optimizer == 'RMSprop':
            self.alpha, self.rms_eps = 0.99, 1e-8
            self.state = dict(square_avg=zeros())
        else:
            self.momentum = 0.9                                               # model.py:161
            self.state = dict(momentum_buffer=zeros())
        self.sqnorm = torch.zeros(4, dtype=torch.float32, device=st.device)
        # the step size lives in a device scalar the optimizer kernel reads at run time: a captured hipGraph follows
        # ReduceLROnPlateau (model.py:164,437) without re-capture
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=st.device)
        self._lr_on_dev = float(lr)
        if world_size > 1:          # identical start on every rank (checkpoints are loaded per process)
            import torch.distributed as dist
            dist.broadcast(st.flat, src=0)
            model.mark_weights_dirty()
        self.last = None
        self._graphs = {}

    def forward_backward(self, x, sem, ins, n_objects, selected_idx=None, injected_s_t=None, capture=None,
                         idx_dev=None, arena_key=None, backward=True, n_obj_dev=None):
        """Forward + backward; gradients land in model.store.grad.  Returns device scalars
        dict(sem=[ce, dice] ([ce, 0, lovasz] for the Lovasz criteria), head=[ins_cost_finite, criterion, ins_ce,
        ins_dice]) and, when the discriminative embedding loss is on, disc=[weighted loss, var, dist, reg, qreg, present
        instances, their pixels, 0].  n_obj_dev: the object counts as int32 [B] on the device (the captured step stages
        them).  backward=False: the training-mode forward alone (batch statistics, sampling, Dropout2d, losses; no
        tape) - the forward-only benchmark line."""
        m = self.model
        E, net, st = m.engine, m.net, m.store
        dev = st.device
        x = x.to(device=dev) if x.dtype == torch.uint8 else x.to(device=dev, dtype=torch.float32)
        sem = sem.to(dev).contiguous()
        ins = ins.to(dev).contiguous()
        if backward:
            st.grad[:st.n_train].zero_()
        E.begin(bn_train=m.training, record=backward,
                key=arena_key or ("train", tuple(x.shape), x.dtype, tuple(ins.shape), ins.dtype,
                                  injected_s_t is not None))
        if getattr(m, "_weights_dirty", True) and E.packer.entries:
            E.packer.pack()
        m._weights_dirty = False
        labels = None
        planes = ins                         # as given: the border term builds its label map from them
        if ins.dtype == torch.uint8:         # compact targets (uint8 planes [B,H,W,K] + uint8 map [B,H,W]): expand on device
            if net.crit.legacy:
                sem, ins = net.collate_targets(sem, ins)
            else:                            # the K-class criterion reads the label map; the head the one-hot
                sem, ins, labels = net.collate_targets(sem, ins, labels=True, onehot=m.use_instance_seg)
        xin = net.input_view(x)
        x_dec, feats = net.unet(xin)
        sem_a = net.sem_head(x_dec)
        m._last_sem = sem_a                  # the step's logits (arena view: read before the next step)
        sem_scal = net.sem_loss(sem_a, sem, labels, planes)
        head_scal = None
        if m.use_instance_seg:
            n_ins = n_objects if isinstance(n_objects, list) else [int(v) for v in n_objects.reshape(-1).tolist()]
            if selected_idx is None and idx_dev is None:
                selected_idx = []
                for k in n_ins:
                    order = list(range(k))
                    random.shuffle(order)
                    selected_idx.append(order)
            sem_map = net.onehot_map(sem)                    # GT.argmax(1) (reseg.py:118) as the fp32 map the head reads
            disc = None
            if net.disc.on:
                disc = dict(n_obj=n_obj_dev if n_obj_dev is not None else
                            torch.tensor(n_ins, dtype=torch.int32, device=dev))
            rec = m.head.forward(x_dec, feats, sem_map, ins, n_ins, True, selected_idx, injected_s_t, capture,
                                 idx_dev=idx_dev, disc=disc)
            m.last_record = rec
            head_scal = rec["scal"]
        if backward:
            E.backward()
        self.last = dict(sem=sem_scal, head=head_scal)
        if m.use_instance_seg and net.disc.on:
            self.last["disc"] = disc["scal"]
        return self.last

    def set_disc_weight(self, weight):
        """A new weight (> 0) of the running discriminative loss, written in place into its device settings: a captured
        step follows without re-capture.  Switching the loss on or off is a new Trainer."""
        self.model.net.disc.set_weight(weight)

    def set_border(self, weight, sigma=None):
        """New values (weight > 0) of the running border term, written in place into its device settings: a captured step
        follows without re-capture.  Switching the term on or off is a new Trainer."""
        self.model.net.crit.set_border_values(weight, sigma)

    @property
    def class_weights(self):
        """The class weights the K-class criterion reads, on the device (ones when none were given); write them in place
        (`.copy_`) and a captured step follows.  None on the shipped criterion, whose kernels take no weights."""
        crit = self.model.net.crit
        return None if crit.legacy else crit.weights

    def sync_lr(self):
        """Host lr -> device scalar (outside any graph; a no-op unless the scheduler changed it)."""
        if self._lr_on_dev != float(self.lr):
            self.lr_dev.fill_(float(self.lr))
            self._lr_on_dev = float(self.lr)

    def apply_update(self):
        """all-reduce (world > 1) -> norm of the averaged gradient -> clip + the optimizer's update, over the updated range:
        parallel.exchange_and_update owns the ordering (the CPU test drives the same function with stand-in kernels)."""
        st = self.model.store
        lib = self.model.engine.lib
        self.sqnorm.zero_()
        lo, n_upd = self.lo, st.n_train - self.lo
        params, S = st.flat[lo:st.n_train], self.state
        tail = (self.sqnorm, float(self.clip))       # ..., gscale, lr_dev, stream follow in every entry

        def sqnorm_fn(grad, n, gscale):
            lib.isa_sqnorm(grad, n, gscale, self.sqnorm, L.stream_ptr())

        def update_fn(grad, n, gscale):
            p, g, end = params, grad, (gscale, self.lr_dev, L.stream_ptr())
            if self.optimizer == 'Adadelta':
                lib.isa_adadelta(p, g, self.sq, self.acc, n, self.lr, self.rho, self.eps, self.wd, *tail, *end)
            elif self.optimizer == 'Adam':
                lib.isa_adam(p, g, S["exp_avg"], S["exp_avg_sq"], S["step"], self._adam_aux, n, self.lr, self.betas[0],
                             self.betas[1], self.adam_eps, self.wd, *tail, *end)
            elif self.optimizer == 'RMSprop':
                lib.isa_rmsprop(p, g, S["square_avg"], n, self.lr, self.alpha, self.rms_eps, self.wd, *tail, *end)
            else:
                lib.isa_sgd(p, g, S["momentum_buffer"], n, self.lr, self.momentum, self.wd, *tail, *end)

        exchange_and_update(st.grad[lo:st.n_train], n_upd, self.world, sqnorm_fn, update_fn, self.clip)
        self.model.mark_weights_dirty()

    def train_step(self, x, sem, ins, n_objects, selected_idx=None, injected_s_t=None, arena_key=None):
        self.sync_lr()
        out = self.forward_backward(x, sem, ins, n_objects, selected_idx, injected_s_t, arena_key=arena_key)
        self.apply_update()
        return out

    # ------------------------------------------------------------------ hipGraph-captured step
    def train_step_graphed(self, x, sem, ins, n_objects, selected_idx=None, injected_s_t=None, forward_only=False):
        """Same step, replayed from a hipGraph: the ~880 launches of forward+backward (+ the fused update when
        world_size == 1) are recorded once per (shapes, iteration count) and replayed, so the GPU never waits
        for the Python launch loop.  Inputs are copied into static device buffers; the per-step host decisions
        (instance order) travel through a small staged index tensor; dropout masks come from torch's graph-safe
        generator.  The first call of a configuration runs eagerly (allocations settle), the second captures.
        With world_size > 1 the RCCL all-reduce and the update stay outside the graph.
        forward_only: capture and replay the training-mode forward alone (no gradients, no update)."""
        m = self.model
        st = m.store
        dev = st.device
        n_ins = [int(v) for v in n_objects.reshape(-1).tolist()]
        from .instance_head import MAX_ITER
        max_iter = min(MAX_ITER, min(n_ins)) if m.use_instance_seg else 0
        if m.use_instance_seg and selected_idx is None:
            selected_idx = []
            for k in n_ins:
                order = list(range(k))
                random.shuffle(order)
                selected_idx.append(order)
        key = (tuple(x.shape), tuple(sem.shape), tuple(ins.shape), max_iter, bool(m.training), self.world,
               m.engine.dtype, injected_s_t is not None, x.dtype == torch.uint8, ins.dtype == torch.uint8, bool(forward_only),
               # the Lovasz criteria have launches of their own (CELovasz three more than Lovasz), and per_image sets
               # their segment geometry
               m.net.crit.criterion if m.net.crit.lovasz else None, m.net.crit.lovasz and m.net.crit.lovasz_per_image,
               # the border term: on / off adds launches and picks the pixel-weighted kernels; w0 and sigma do not
               m.net.crit.border_key(),
               # the discriminative loss: on / off adds launches, form and norm pick kernels; weight and deltas do not
               m.net.disc.key() if m.use_instance_seg else None)
        disc_on = m.use_instance_seg and m.net.disc.on
        slot = self._graphs.get(key)
        akey = ("train_graph",) + key            # the captured configuration owns its arena (frozen after capture)
        self.sync_lr()
        def eager(arena_key=None):
            if forward_only:
                return self.forward_backward(x, sem, ins, n_objects, selected_idx, injected_s_t, arena_key=arena_key,
                                             backward=False)
            return self.train_step(x, sem, ins, n_objects, selected_idx=selected_idx, injected_s_t=injected_s_t,
                                   arena_key=arena_key)
        if slot is None:                         # first sight: eager step, remember the configuration
            self._graphs[key] = dict(state="warm")
            return eager(akey)
        if slot["state"] == "eager":
            return eager()
        if slot["state"] == "warm":
            slot["x"] = torch.empty(tuple(x.shape), dtype=torch.uint8 if x.dtype == torch.uint8 else torch.float32,
                                    device=dev)
            slot["sem"] = torch.empty(tuple(sem.shape), dtype=sem.dtype, device=dev)
            slot["ins"] = torch.empty(tuple(ins.shape), dtype=ins.dtype, device=dev)
            slot["idx"] = torch.zeros((max(max_iter, 1), x.shape[0]), dtype=torch.int32, device=dev)
            slot["idx_pin"] = torch.zeros((max(max_iter, 1), x.shape[0]), dtype=torch.int32).pin_memory()
            slot["inj"] = None if injected_s_t is None else [torch.zeros_like(t) for t in injected_s_t[:max_iter]]
            if disc_on:                          # the object counts the discriminative loss reads on the device
                slot["nobj"] = torch.zeros(x.shape[0], dtype=torch.int32, device=dev)
                slot["nobj_pin"] = torch.zeros(x.shape[0], dtype=torch.int32).pin_memory()
            self._stage(slot, x, sem, ins, selected_idx, max_iter, injected_s_t, n_ins)
            before = dict(st.int_buffers)
            g = torch.cuda.CUDAGraph()
            try:
                # thread_local: the RCCL watchdog thread may query events while this thread captures
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    out = self.forward_backward(slot["x"], slot["sem"], slot["ins"], n_ins, idx_dev=slot["idx"],
                                                injected_s_t=slot["inj"], arena_key=akey, backward=not forward_only,
                                                n_obj_dev=slot.get("nobj"))
                    if self.world == 1 and not forward_only:
                        self.apply_update()
                m.engine.freeze_arena()
            except Exception as e:                 # capture refused (driver / collective state): stay eager, loudly
                import sys
                print("[isa_amd] hipGraph capture failed (%s: %s); this configuration runs eagerly" %
                      (type(e).__name__, e), file=sys.stderr, flush=True)
                torch.cuda.synchronize()
                st.int_buffers.update(before)
                slot["state"] = "eager"
                return eager()
            # capture only records: undo its host-side counters, replay() below performs the step
            slot["bumps"] = {k: v - before[k] for k, v in st.int_buffers.items() if v != before[k]}
            st.int_buffers.update(before)
            slot.update(state="ready", graph=g, out=out)
        else:
            self._stage(slot, x, sem, ins, selected_idx, max_iter, injected_s_t, n_ins)
        slot["graph"].replay()
        for k, v in slot["bumps"].items():
            st.int_buffers[k] += v
        if not forward_only:
            if self.world > 1:
                self.apply_update()
            m.mark_weights_dirty()
        self.last = slot["out"]
        return self.last

    def static_inputs(self):
        """(x, sem, ins) input buffers of the captured graphs, most recent configuration first: a data pipeline can
        write the next batch straight into them (H2D or a device-side producer) and pass these same tensors to
        train_step_graphed, which then replays without any staging copy."""
        return [(s["x"], s["sem"], s["ins"]) for s in reversed(list(self._graphs.values())) if s.get("state") == "ready"]

    def _stage(self, slot, x, sem, ins, selected_idx, max_iter, injected_s_t=None, n_ins=None):
        if slot.get("nobj") is not None:
            slot["nobj_pin"].copy_(torch.tensor(n_ins, dtype=torch.int32))
            slot["nobj"].copy_(slot["nobj_pin"], non_blocking=True)
        if slot.get("inj") is not None:          # parity runs: glimpse points fixed from outside
            for dst, src in zip(slot["inj"], injected_s_t):
                dst.copy_(src, non_blocking=True)
        # a caller that fills the graph's own input buffers (static_inputs) skips the device-to-device copies
        if x is not slot["x"]:
            slot["x"].copy_(x, non_blocking=True)
        if sem is not slot["sem"]:
            slot["sem"].copy_(sem, non_blocking=True)
        if ins is not slot["ins"]:
            slot["ins"].copy_(ins, non_blocking=True)
        if max_iter > 0:
            n = slot["x"].shape[0]
            slot["idx_pin"].copy_(self.model.head.order_tensor(selected_idx, max_iter, n))
            slot["idx"].copy_(slot["idx_pin"], non_blocking=True)
