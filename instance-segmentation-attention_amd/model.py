"""Trainer / predictor mirror of the reference's `Model` (code/lib/model.py): same constructor
arguments, `fit(...)` and `predict(images)` semantics, best-validation checkpointing of the
`state_dict` (model.py:437-446), ReduceLROnPlateau on the validation ins_dice_loss (model.py:428-437),
CSV logs (model.py:366-372,458-461).  Differences, all host-side: no visdom plots, no pickles to a
hard-coded path, no debug JPEGs; compute is the HIP engine (Trainer / ReSeg), never torch ops.
"""
import os

import numpy as np
import torch

from . import parallel
from .reseg import ReSeg
from .trainer import Trainer


class Model(object):
    def __init__(self, dataset, model_name, n_classes, max_n_objects, use_instance_segmentation=False,
                 use_coords=False, load_model_path='', load_decoder_model_path='', usegpu=True, use_wae=False,
                 wae_opt=None, dtype=torch.float32):
        self.dataset, self.model_name = dataset, model_name
        self.n_classes, self.max_n_objects = n_classes, max_n_objects
        self.use_instance_segmentation = use_instance_segmentation
        self.use_coords, self.load_model_path, self.usegpu, self.use_wae = use_coords, load_model_path, usegpu, use_wae
        assert self.dataset in ['CVPPP', ]                                    # model.py:39
        assert self.model_name in ['ReSeg', 'StackedRecurrentHourglass']      # model.py:40
        assert self.model_name == 'ReSeg', "only ReSeg is live at HEAD (SURVEY.md §0-2)"
        assert usegpu, "this build has no CPU path"
        # data parallel: one process per GPU under torch.distributed.run; a single process otherwise (parallel.py)
        self.world, self.rank, self.local_rank = parallel.env_world()
        self.model = ReSeg(self.n_classes, self.use_instance_segmentation, pretrained=True,
                           use_coordinates=self.use_coords, use_wae=use_wae, usegpu=True, dtype=dtype)
        self.__load_weights()
        self.trainer = None
        self.lr_scheduler = None
        # fit(): also segment and score every validation minibatch (SBD, |DiC|, FG Dice -> validation_scores.log)
        self.val_scores = False
        # fit(): also score the semantic prediction of every validation minibatch (confusion matrix on the device; mIoU,
        # pixel accuracy, mean Dice of the epoch total -> validation_sem_scores.log)
        self.val_sem_scores = False
        # fit(): the options of the Lovasz and CELovasz criteria (lovasz_softmax's per_image and only_present)
        self.lovasz_per_image = False
        self.lovasz_only_present = False

    def __load_weights(self):
        if self.load_model_path != '':
            assert os.path.isfile(self.load_model_path), 'Model : {} does not exists!'.format(self.load_model_path)
            print('Loading model from {}'.format(self.load_model_path))
            # model.py:62-79: update the model's own dict, tolerate partial files.  weights_only: no code runs
            state = self.model.state_dict()
            loaded = torch.load(self.load_model_path, map_location='cpu', weights_only=True)
            state.update({k: v for k, v in loaded.items() if k in state})     # e.g. instance stems -> sem-only net
            self.model.load_state_dict(state)

    # ------------------------------------------------------------------ training
    def __define_optimizer(self, learning_rate, weight_decay, lr_drop_factor, lr_drop_patience, clip_grad_norm,
                           optimizer='Adadelta', criterion='Multi', class_weights=None, optimize_bg=False,
                           train_cnn=True, lovasz_per_image=False, lovasz_only_present=False, disc=None):
        assert optimizer in ['RMSprop', 'Adam', 'Adadelta', 'SGD']            # model.py:147
        # the criterion of __define_criterion (model.py:102-133): CE(weight) and / or Dice(optimize_bg, weight)
        self.trainer = Trainer(self.model, world_size=self.world, lr=learning_rate, weight_decay=weight_decay,
                               clip_grad_norm=clip_grad_norm, criterion=criterion, class_weights=class_weights,
                               optimize_bg=optimize_bg, optimizer=optimizer, train_cnn=train_cnn,
                               lovasz_per_image=lovasz_per_image, lovasz_only_present=lovasz_only_present, **(disc or {}))
        self._plateau = dict(best=float('inf'), bad=0, factor=lr_drop_factor, patience=lr_drop_patience)

    def __plateau_step(self, val):                   # torch ReduceLROnPlateau(mode='min') semantics, rel 1e-4
        p = self._plateau
        if val < p['best'] * (1 - 1e-4):
            p['best'], p['bad'] = val, 0
        else:
            p['bad'] += 1
        if p['bad'] > p['patience']:
            self.trainer.lr *= p['factor']
            p['bad'] = 0
            if self.rank == 0:
                print('Reducing learning rate to {}'.format(self.trainer.lr))

    def __minibatch(self, batch, mode):
        assert mode in ['training', 'test'], 'Mode must be either "training" or "test"'      # model.py:193
        images, sem, ins, n_objects = batch
        if mode == 'training':
            self.model.train()
            # hipGraph replay of the step (ISA_GRAPH=0: eager launch loop)
            step = self.trainer.train_step if os.environ.get('ISA_GRAPH', '1') == '0' else self.trainer.train_step_graphed
            out = step(images, sem, ins, n_objects)
        else:
            self.model.eval()
            with torch.no_grad():
                if self.use_instance_segmentation:
                    sem_out, sem_arg, ins_cost, crit, ce, dice = self.model(False, images, sem, ins, n_objects.unsqueeze(1))
                    row = {'INS Cost': ins_cost, 'Criterion': crit, 'ins_ce_loss': ce, 'ins_dice_loss': dice}
                else:
                    self.model(False, images)
                    row = {}
                if sem.dtype == torch.uint8:              # compact targets: one-hot on the device (isa_collate_targets)
                    sem, _ = self.model.net.collate_targets(sem, ins)
                # the reference logs CE / Dice in validation too (model.py:255-269); the border term needs the planes
                costs = self.model.sem_costs(sem, ins if self.model.net.crit.border_on else None)
                row.update(self.__sem_row(costs))
                if self.val_sem_scores:                   # before the next forward: the logits live in this step's arena
                    _, conf = self.model.score_semantic(sem, check=False)
                    row['sem_conf'] = (conf.sum(0), self.model.last_sem_oob.sum())
                if self.val_scores and self.use_instance_segmentation:
                    row['scores'] = self.__score_batch(batch, self.max_n_objects, check=False)
            return row
        row = self.__sem_row(out['sem'])
        h = out['head']
        if h is not None:                                 # semantic-only models have no instance head (model.py:244)
            row.update({'INS Cost': h[0] + float('nan'), 'Criterion': h[1].clone(), 'ins_ce_loss': h[2].clone(),
                        'ins_dice_loss': h[3].clone()})
        if 'disc' in out:                                 # the discriminative embedding loss, weight included
            row['Disc Cost'] = out['disc'][0].clone()
        return row

    def __instances(self, images, max_objects, method, bandwidth, n_objects):
        """(sem_argmax, labels, n_objects) of one batch by `method`: 'attention' (ReSeg.segment), or 'meanshift' / 'kmeans'
        on the instance embedding (ReSeg.segment_embedding; at most 32 instances)."""
        m = self.model
        if method == 'attention':
            _, sem_arg, labels, count = m.segment(images.contiguous(), max_objects)
        elif method in ('meanshift', 'kmeans'):
            if method == 'kmeans' and n_objects is None:
                raise ValueError("method 'kmeans' needs n_objects")
            _, sem_arg, labels, count = m.segment_embedding(images.contiguous(), method=method, bandwidth=bandwidth,
                                                            max_objects=min(int(max_objects), 32), n_objects=n_objects)
        else:
            raise ValueError("method must be 'attention', 'meanshift' or 'kmeans', got %r" % (method,))
        return sem_arg, labels, count

    def __score_batch(self, batch, max_objects, check, clean=None, method='attention', bandwidth=None, fill=False,
                      fill_max_dist=None, select=None):
        """segment() + score_instances() of one loader batch: the device tensor [B,8], and the number of pixels whose
        label the histograms do not hold (a device scalar: the callers read it with their one copy and raise).
        clean: keyword arguments of ReSeg.clean_instances, applied to the labels before they are scored; fill: then the
        unlabelled foreground of the predicted class map goes to the nearest instance (ReSeg.fill_instances); select: then
        keyword arguments of ReSeg.select_instances."""
        images, sem, ins, n_objects = batch
        m = self.model
        sem_arg, labels, count = self.__instances(images, max_objects, method, bandwidth, n_objects)
        if clean is not None:
            labels, count, _ = m.clean_instances(labels, max_objects=max_objects, **clean)
        if fill:
            labels, _ = m.fill_instances(labels, m.class_map(), fill_max_dist)
        if select is not None:
            labels, count, _ = m.select_instances(labels, max_objects=max_objects, **select)
        out = m.score_instances(labels, count, ins, n_objects, sem_arg, sem, max_objects=max_objects, check=check)
        return out, m.last_score_oob.sum()

    @staticmethod
    def __refuse_oob(n_oob):
        if n_oob:
            raise ValueError("%d pixels carry a label outside the score histograms (ReSeg.score_instances: at most 256 ids "
                             "a side and 16384 pairs)" % n_oob)

    @staticmethod
    def __score_means(per_image):
        """Means of SBD, |DiC| and FG Dice over the images whose value is not NaN, as evaluate.py's main takes them over
        the images it scored; device tensors (means [3], number of NaN images of the SBD column)."""
        cols = per_image[:, [2, 5, 6]]
        ok = ~torch.isnan(cols)
        means = torch.where(ok, cols, torch.zeros_like(cols)).sum(0) / ok.sum(0)
        return means, (~ok[:, 0]).sum()

    def __sem_row(self, costs):
        """Only the terms the criterion computes, as the reference's out_metrics (model.py:255-269)."""
        crit = self.model.net.crit
        row = {}
        if crit.ce:
            row['CE Cost'] = costs[0].clone()
        if crit.dice:
            row['Dice Cost'] = costs[1].clone()
        if crit.lovasz:
            row['Lovasz Cost'] = costs[2].clone()
        return row

    def fit(self, criterion_type, delta_var, delta_dist, norm, learning_rate, weight_decay, clip_grad_norm,
            lr_drop_factor, lr_drop_patience, optimize_bg, optimizer, train_cnn, n_epochs, class_weights,
            train_loader, test_loader, model_save_path, debug, lovasz_per_image=None, lovasz_only_present=None,
            border_weight=0.0, border_sigma=5.0, disc_weight=0.0, disc_form='reference'):
        """model.py:359-460.  delta_var, delta_dist, norm: the parameters of the reference's DiscriminativeLoss
        (model.py:109-115, which it builds and never calls); here the loss trains the instance embedding when
        disc_weight > 0, in the form disc_form ('reference' | 'full', ReSeg.discriminative_loss).
        border_weight > 0 weighs the cross-entropy of every pixel by the U-Net border map of the step's instance targets,
        1 + border_weight * exp(-(d1 + d2)^2 / (2 border_sigma^2)), computed on the device (ReSeg.border_weights)."""
        assert criterion_type in ['CE', 'Dice', 'Multi', 'Lovasz', 'CELovasz']  # model.py:364, and the Lovasz criteria
        if lovasz_per_image is None:
            lovasz_per_image = self.lovasz_per_image
        if lovasz_only_present is None:
            lovasz_only_present = self.lovasz_only_present
        main = self.rank == 0                   # only rank 0 writes logs and checkpoints (parallel.py: policy)
        tlog = vlog = slog = mlog = None
        scoring = bool(self.val_scores) and self.use_instance_segmentation
        if main:
            os.makedirs(model_save_path, exist_ok=True)
            tlog = open(os.path.join(model_save_path, 'training.log'), 'w')
            vlog = open(os.path.join(model_save_path, 'validation.log'), 'w')
            tlog.write('Epoch,Cost\n'); vlog.write('Epoch,Cost\n')
            if scoring:
                slog = open(os.path.join(model_save_path, 'validation_scores.log'), 'w')
                slog.write('Epoch,SBD,DiC,FG Dice\n')
            if self.val_sem_scores:
                mlog = open(os.path.join(model_save_path, 'validation_sem_scores.log'), 'w')
                mlog.write('Epoch,mIoU,PixelAcc,mDice\n')
        self.__define_optimizer(learning_rate, weight_decay, lr_drop_factor, lr_drop_patience, clip_grad_norm, optimizer,
                                criterion_type, class_weights, optimize_bg, train_cnn, lovasz_per_image,
                                lovasz_only_present,
                                dict(disc_weight=disc_weight, delta_var=delta_var, delta_dist=delta_dist, disc_norm=norm,
                                     disc_form=disc_form, border_weight=border_weight, border_sigma=border_sigma))
        best_val_cost = np.inf
        if os.environ.get('ISA_PREFETCH', '1') != '0':      # batch i+1 uploads on a side stream while step i runs
            from .data import DevicePrefetcher
            train_loader, test_loader = DevicePrefetcher(train_loader), DevicePrefetcher(test_loader)
        for epoch in range(n_epochs):
            tr = [self.__minibatch(b, 'training') for b in train_loader]
            # every rank validates the same model: average the per-rank running estimates first
            parallel.sync_buffers(self.model.store, self.model.head.baseline if self.use_instance_segmentation else None,
                                  self.world)
            if self.world > 1:
                self.model.engine.eval_bn_stale = True      # the running statistics were rewritten: cached eval constants are old
            va = [self.__minibatch(b, 'test') for b in test_loader]
            # an empty loader (a validation set smaller than one batch per rank under a dropping sampler) must not take the
            # epoch down on every rank: its mean is NaN and the plateau scheduler sees the training cost instead
            mean = lambda rows, k: float(torch.stack([r[k].float() for r in rows]).mean()) if rows else float("nan")
            # the cost that drives the plateau scheduler and checkpointing (model.py:425-434)
            if self.use_instance_segmentation:
                key = 'ins_dice_loss'
            elif criterion_type in ['Lovasz', 'CELovasz']:
                key = 'Lovasz Cost'
            elif criterion_type in ['Dice', 'Multi']:
                key = 'Dice Cost'
            else:
                key = 'CE Cost'
            # rank-averaged costs: the plateau scheduler must take the same decision on every rank
            train_cost = parallel.mean_over_ranks(mean(tr, key), self.world)
            val_cost = parallel.mean_over_ranks(mean(va, key), self.world)
            if val_cost != val_cost:
                val_cost = train_cost
            if main:
                print('Epoch : [{}/{}]  train {} {:.5f} | val {:.5f}'.format(epoch, n_epochs, key, train_cost, val_cost))
            self.__plateau_step(val_cost)
            if val_cost <= best_val_cost:                                       # model.py:439-446
                best_val_cost = val_cost
                if main:
                    torch.save(self.model.state_dict(), os.path.join(
                        model_save_path, 'model_{}_{}_{}.pth'.format(epoch, val_cost, self.trainer.lr)))
            if main:
                tlog.write('{},{}\n'.format(epoch, train_cost)); vlog.write('{},{}\n'.format(epoch, val_cost))
                tlog.flush(); vlog.flush()
            if scoring:
                # per-epoch means over this rank's validation images, then over the ranks, as the costs are
                rows = [r['scores'][0] for r in va]
                means = [float('nan')] * 3
                if rows:
                    got = torch.cat([self.__score_means(torch.cat(rows))[0],
                                     torch.stack([r['scores'][1] for r in va]).sum().double().view(1)]).tolist()
                    self.__refuse_oob(int(got[3]))
                    means = got[:3]
                means = [parallel.mean_over_ranks(v, self.world) for v in means]
                if main:
                    slog.write('{},{},{},{}\n'.format(epoch, *means)); slog.flush()
            if self.val_sem_scores:
                # the epoch-total confusion matrix: summed over this rank's minibatches, then over the ranks, then scored
                K = self.n_classes
                total = torch.zeros(K * K + 1, dtype=torch.int64, device=self.model.store.device)
                for r in va:
                    total[:K * K] += r['sem_conf'][0].reshape(-1)
                    total[K * K] += r['sem_conf'][1]
                total = parallel.sum_over_ranks(total, self.world)
                got = torch.cat([self.model.semantic_scores(total[:K * K].view(K, K))[:3], total[K * K:].double()]).tolist()
                if int(got[3]):
                    raise ValueError("%d validation pixels carry a label outside the K = %d classes" % (int(got[3]), K))
                if main:
                    mlog.write('{},{},{},{}\n'.format(epoch, got[1], got[0], got[2])); mlog.flush()
        if main:
            tlog.close(); vlog.close()
            if slog is not None:
                slog.close()
            if mlog is not None:
                mlog.close()

    # ------------------------------------------------------------------ inference (model.py:466-499)
    def predict(self, images):
        assert len(images.size()) == 4  # b, c, h, w
        self.model.eval()
        m = self.model
        if m.use_instance_seg:
            # the shipped ModelSettings hit an UnboundLocalError here (reseg.py:126); the only working
            # inference mode is the semantic one — same contract, clearer message
            raise RuntimeError("predict() needs a model built with use_instance_segmentation=False")
        m(False, images.contiguous())
        return m.net.softmax_nchw(m._last_sem).cpu()                          # softmax over classes (model.py:486)

    def predict_classes(self, images):
        """Class ids of a semantic-only model: a host uint8 tensor [b,h,w], the arg-max of predict()'s softmax (first
        maximum wins), taken on the device from the logits (ReSeg.class_map) - one byte per pixel comes down, not the K
        fp32 probabilities."""
        assert len(images.size()) == 4  # b, c, h, w
        self.model.eval()
        m = self.model
        if m.use_instance_seg:
            raise RuntimeError("predict_classes() needs a model built with use_instance_segmentation=False")
        with torch.no_grad():
            m(False, images.contiguous())
            return m.class_map().cpu()

    @staticmethod
    def __clean_arguments(min_area, keep, connectivity):
        """None when the defaults ask for no clean-up (then nothing of it runs), else ReSeg.clean_instances' keywords.
        keep=None with a min_area above 1 drops small pieces and keeps everything else apart: 'all'."""
        if keep not in (None, 'largest', 'all'):
            raise ValueError("keep must be None, 'largest' or 'all', got %r" % (keep,))
        if connectivity not in (4, 8):
            raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
        if keep is None and int(min_area) <= 1:
            return None
        return {'keep': keep or 'all', 'connectivity': connectivity, 'min_area': int(min_area)}

    @staticmethod
    def __select_arguments(order, clear_border, max_area):
        """None when the defaults ask for no selection (then nothing of it runs), else ReSeg.select_instances' keywords."""
        if order not in (None, 'label', 'area', 'raster'):
            raise ValueError("order must be None, 'label', 'area' or 'raster', got %r" % (order,))
        if max_area is not None and int(max_area) < 1:
            raise ValueError("max_area must be positive or None, got %r" % (max_area,))
        if order is None and not clear_border and max_area is None:
            return None
        return {'order': order or 'label', 'clear_border': bool(clear_border), 'max_area': max_area}

    def predict_instances(self, images, max_objects=None, *, min_area=0, keep=None, connectivity=8, method='attention',
                          bandwidth=None, n_objects=None, fill=False, fill_max_dist=None, order=None, clear_border=False,
                          max_area=None):
        """Instance inference for models built with use_instance_segmentation=True (ReSeg.segment; the reference's own
        instance prediction is dead at HEAD).  images: [b,21,h,w] float or raw uint8 RGB [b,h,w,3].  Returns host tensors
        (fg_prob [b,h,w] = softmax probability of the foreground class, labels uint8 [b,h,w] with 0 = no instance,
        n_objects int32 [b]); at most max_objects (default: the constructor's max_n_objects) instances per image.
        keep='largest' | 'all' and / or min_area > 1 clean the label map on the device before it comes down
        (ReSeg.clean_instances: the largest connected piece of every instance, or every piece as an instance of its own;
        pieces under min_area pixels dropped; connectivity 4 or 8).  With the defaults none of that runs.
        method='meanshift' | 'kmeans' takes the instances from clusters of the instance embedding instead of the attention
        decoder (ReSeg.segment_embedding, at most 32 per image): mean-shift of radius bandwidth (default 1.5 = delta_dist),
        or k-means with the object counts n_objects [b].
        fill=True gives, after the clean-up, every foreground pixel of the predicted class map that is still 0 to the nearest
        instance (ReSeg.fill_instances), within fill_max_dist pixels when that is given.  Off by default.
        order='label' | 'area' | 'raster', clear_border=True and / or max_area then filter and renumber the instances by
        their measurements (ReSeg.select_instances, after the clean-up and the fill): instances that touch the image edge or
        exceed max_area pixels are dropped, and the rest are numbered by old label, largest first, or by first pixel.  Off
        by default."""
        fg_prob, labels, n_objects = self.__predict_instances(
            images, max_objects, min_area=min_area, keep=keep, connectivity=connectivity, method=method, bandwidth=bandwidth,
            n_objects=n_objects, fill=fill, fill_max_dist=fill_max_dist, order=order, clear_border=clear_border,
            max_area=max_area)
        return fg_prob.cpu(), labels.cpu(), n_objects.cpu()

    def __predict_instances(self, images, max_objects=None, *, min_area=0, keep=None, connectivity=8, method='attention',
                            bandwidth=None, n_objects=None, fill=False, fill_max_dist=None, order=None, clear_border=False,
                            max_area=None):
        """predict_instances' answer as device tensors."""
        assert len(images.size()) == 4
        m = self.model
        if not m.use_instance_seg:
            raise RuntimeError("predict_instances() needs a model built with use_instance_segmentation=True")
        clean = self.__clean_arguments(min_area, keep, connectivity)
        select = self.__select_arguments(order, clear_border, max_area)
        m.eval()
        max_objects = self.max_n_objects if max_objects is None else max_objects
        _, labels, n_objects = self.__instances(images, max_objects, method, bandwidth, n_objects)
        if clean is not None:
            labels, n_objects, _ = m.clean_instances(labels, max_objects=max_objects, **clean)
        if fill:
            labels, _ = m.fill_instances(labels, m.class_map(), fill_max_dist)
        if select is not None:
            labels, n_objects, _ = m.select_instances(labels, max_objects=max_objects, **select)
        return m.net.softmax_nchw(m._last_sem)[:, 1], labels, n_objects

    def measure_instances(self, images, **predict_kwargs):
        """predict_instances(images, **predict_kwargs) and the measurements of what it found: (fg_prob, labels, n_objects,
        props), props a list with one float64 ndarray [n_objects[b], 24] per image whose row k describes instance k + 1 in
        the columns reseg.PROPS_COLUMNS (ReSeg.instance_properties, taken on the device at model resolution; the colour
        means are those of raw uint8 RGB input and NaN for any other input)."""
        m = self.model
        fg_prob, labels, n_objects = self.__predict_instances(images, **predict_kwargs)
        raw = images if images.dtype == torch.uint8 and tuple(images.shape) == tuple(labels.shape) + (3,) else None
        props = m.instance_properties(labels, raw).cpu().numpy()
        counts = n_objects.cpu()
        rows = [props[b, 1:1 + int(counts[b])] for b in range(props.shape[0])]
        return fg_prob.cpu(), labels.cpu(), counts, rows

    def predict_polygons(self, images, **predict_kwargs):
        """predict_instances(images, **predict_kwargs) and the outlines of what it found: (fg_prob, labels, n_objects,
        polygons), polygons a list per image of {'label', 'outer': int16 [k,2], 'holes': [int16 [k,2], ...]} in
        model-resolution pixel-corner coordinates (ReSeg.polygons, traced on the device under the clean-up's connectivity,
        8 by default)."""
        m = self.model
        fg_prob, labels, n_objects = self.__predict_instances(images, **predict_kwargs)
        polys = m.polygons(labels, connectivity=predict_kwargs.get('connectivity', 8))
        return fg_prob.cpu(), labels.cpu(), n_objects.cpu(), polys

    def predict_components(self, images, *, min_area=1, connectivity=8, max_objects=None):
        """The count-the-blobs baseline, for any model (no instance head is run): the connected components of the predicted
        class map (class 0 = background; pixels of different classes never join) with at least min_area pixels, numbered in
        raster order (ReSeg.split_components).  Returns what predict_instances returns: host tensors (fg_prob [b,h,w] = the
        softmax probability of not being background, labels uint8 [b,h,w], n_objects int32 [b]); at most max_objects
        (default: the constructor's max_n_objects, 1..255) objects per image."""
        assert len(images.size()) == 4
        m = self.model
        m.eval()
        max_objects = self.max_n_objects if max_objects is None else max_objects
        with torch.no_grad():
            m._semantic_logits(images.to(m.store.device).contiguous())
            labels, n_objects, _ = m.split_components(m.class_map(), connectivity=connectivity, min_area=min_area,
                                                      max_objects=max_objects)
            prob = m.net.softmax_nchw(m._last_sem)
            fg_prob = prob[:, 1] if prob.shape[1] == 2 else 1.0 - prob[:, 0]
        return fg_prob.cpu(), labels.cpu(), n_objects.cpu()

    def evaluate(self, loader, max_objects=None, *, min_area=0, keep=None, connectivity=8, method='attention',
                 bandwidth=None, fill=False, fill_max_dist=None, order=None, clear_border=False, max_area=None):
        """Scores of ground-truth-free instance inference over a loader of (images, sem, ins, n_objects) batches, either
        target form: every batch is segmented (ReSeg.segment, at most max_objects instances per image; default: the
        constructor's max_n_objects) and scored on the device (ReSeg.score_instances); one device-to-host copy at the end.
        Returns {'SBD', '|DiC|', 'FG Dice', 'n_images', 'n_skipped', 'per_image'}: per_image is the float64 ndarray
        [N,8] of score_instances, the three means are taken over the images whose value is not NaN (evaluate.py's main
        averages the images it scored), n_skipped counts the images whose SBD is NaN (neither map holds an object).
        min_area / keep / connectivity: the clean-up of predict_instances, applied to every label map before it is scored
        (with the defaults none of it runs).  fill / fill_max_dist: predict_instances' fill, after the clean-up.
        order / clear_border / max_area: predict_instances' selection by measurement, after both (off by default).
        method='meanshift' | 'kmeans': the instances come from clusters of the instance embedding (predict_instances);
        'kmeans' is given every batch's ground-truth object counts - the reference's protocol, a count supplied.
        It scores what the loader yields on THIS rank; reducing over ranks is left to the caller."""
        m = self.model
        if not m.use_instance_seg:
            raise RuntimeError("evaluate() needs a model built with use_instance_segmentation=True")
        clean = self.__clean_arguments(min_area, keep, connectivity)
        select = self.__select_arguments(order, clear_border, max_area)
        m.eval()
        max_objects = self.max_n_objects if max_objects is None else max_objects
        rows = [self.__score_batch(b, max_objects, check=False, clean=clean, method=method, bandwidth=bandwidth, fill=fill,
                                   fill_max_dist=fill_max_dist, select=select) for b in loader]
        if not rows:
            nan = float('nan')
            return {'SBD': nan, '|DiC|': nan, 'FG Dice': nan, 'n_images': 0, 'n_skipped': 0,
                    'per_image': np.zeros((0, 8))}
        per_image = torch.cat([r[0] for r in rows])
        means, skipped = self.__score_means(per_image)
        n_oob = torch.stack([r[1] for r in rows]).sum()
        host = torch.cat([per_image.reshape(-1), means, skipped.double().view(1), n_oob.double().view(1)]).cpu().numpy()
        self.__refuse_oob(int(host[-1]))
        per = host[:-5].reshape(-1, 8)
        return {'SBD': float(host[-5]), '|DiC|': float(host[-4]), 'FG Dice': float(host[-3]), 'n_images': per.shape[0],
                'n_skipped': int(host[-2]), 'per_image': per}

    def evaluate_semantic(self, loader):
        """Semantic scores over a loader of (images, sem, ins, n_objects) batches, either target form (sem uint8 [B,H,W]
        or one-hot int64 [B,K,H,W]), for semantic-only models and for the K = 2 semantic head of instance models: per
        batch the backbone and the semantic head run and the confusion matrices are counted on the device
        (ReSeg.score_semantic); the matrices are summed on the device; one device-to-host copy at the end.
        Returns {'mIoU', 'Pixel Acc', 'mDice', 'IoU' [K], 'Dice' [K], 'confusion' int64 [K,K], 'n_images', 'per_image'
        float64 [N, 4+2K]}.  The headline figures are those of the dataset-total confusion matrix (the usual
        definition: the mean over the classes present of the IoU of the summed matrix), not means of per-image values;
        per_image holds the rows of score_semantic.  An empty loader gives NaN and 0.  A label >= K raises ValueError.
        It scores what the loader yields on THIS rank; reducing over ranks is left to the caller
        (parallel.sum_over_ranks on 'confusion', then ReSeg.semantic_scores)."""
        m = self.model
        m.eval()
        K = self.n_classes
        dev = m.store.device
        total = torch.zeros((K, K), dtype=torch.int64, device=dev)
        n_oob = torch.zeros((), dtype=torch.int64, device=dev)
        rows = []
        for images, sem, _ins, _n in loader:
            m._semantic_logits(images.to(dev).contiguous())
            scores, conf = m.score_semantic(sem, check=False)
            rows.append(scores)
            total += conf.sum(0)
            n_oob += m.last_sem_oob.sum()
        per_image = torch.cat(rows) if rows else torch.zeros((0, 4 + 2 * K), dtype=torch.float64, device=dev)
        head = m.semantic_scores(total)
        host = torch.cat([per_image.reshape(-1), head, total.reshape(-1).double(), n_oob.double().view(1)]).cpu().numpy()
        if int(host[-1]):
            raise ValueError("%d pixels carry a label outside the K = %d classes 0..%d" % (int(host[-1]), K, K - 1))
        w = 4 + 2 * K
        n_img = per_image.shape[0]
        head_h = host[n_img * w:(n_img + 1) * w]
        confusion = host[(n_img + 1) * w:-1].astype(np.int64).reshape(K, K)        # counts below 2^53: exact in double
        return {'mIoU': float(head_h[1]), 'Pixel Acc': float(head_h[0]), 'mDice': float(head_h[2]),
                'IoU': head_h[4:4 + K].copy(), 'Dice': head_h[4 + K:].copy(), 'confusion': confusion,
                'n_images': n_img, 'per_image': host[:n_img * w].reshape(n_img, w).copy()}
