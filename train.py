#!/usr/bin/env python3
"""train.py — entry point with the reference's flags (code/train.py:18-37) on the MI355X engine.
The reference trains from an LMDB that is not in its repository; this runs the same loop on synthetic
collated batches (data.py) unless a loader is plugged in.  Hyper-parameters: settings/CVPPP/training_settings.py.

Single GPU:   python train.py --batchsize 8
Data parallel (BASELINE configs[3]: bs=64, 512x512, 8 GPUs; one process per GPU, RCCL gradient all-reduce):
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \
         train.py --batchsize 64 --size 512
--batchsize is the GLOBAL batch (the reference's flag, one process there); each rank takes batchsize / world images of
its own data shard (seeded per rank), only rank 0 logs and writes checkpoints (isa_amd/parallel.py: policy)."""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--model', default='', help="Filepath of trained model (to continue training) [Default: '']")
    parser.add_argument('--usegpu', action='store_true', default=True, help='Enables the GPU [always on in this build]')
    parser.add_argument('--nepochs', type=int, default=800, help='Number of epochs to train for [Default: 800]')
    parser.add_argument('--batchsize', type=int, default=2, help='Batch size [Default: 2]')
    parser.add_argument('--debug', action='store_true', help='Activates debug mode [Default: False]')
    parser.add_argument('--nworkers', type=int, default=2, help='accepted for compatibility (synthetic data needs none)')
    parser.add_argument('--dataset', type=str, default='CVPPP', help='Name of the dataset which is "CVPPP"')
    parser.add_argument('--iters-per-epoch', type=int, default=8)
    parser.add_argument('--size', type=int, default=256, help='image height = width (the reference hard-codes 256, config.py:1)')
    parser.add_argument('--dtype', default='bf16', choices=['bf16', 'f32'])
    parser.add_argument('--compact-targets', action='store_true',
                        help='loader yields uint8 targets (sem [B,H,W], ins [B,H,W,32]); expanded on the device')
    parser.add_argument('--data', default='', help='directory holding <data>/training-lmdb and <data>/validation-lmdb record '
                        'stores (the reference\'s key schema over a directory: isa_amd/records.py); default: synthetic batches')
    parser.add_argument('--out', default=os.path.join(ROOT, 'models', 'CVPPP', 'run'))
    # the semantic criterion (settings/CVPPP/training_settings.py: CRITERION, CLASS_WEIGHTS, OPTIMIZE_BG; data_settings.py:
    # N_CLASSES); the defaults are the shipped settings
    parser.add_argument('--criterion', default='Multi', choices=['CE', 'Dice', 'Multi', 'Lovasz', 'CELovasz'])
    parser.add_argument('--lovasz-per-image', action='store_true', help='Lovasz / CELovasz: the loss per image, then the mean '
                        '(lovasz_softmax per_image; Model.lovasz_per_image)')
    parser.add_argument('--lovasz-present', action='store_true', help='Lovasz / CELovasz: average only the classes present in '
                        'the ground truth (lovasz_softmax only_present; Model.lovasz_only_present)')
    # the discriminative loss on the instance embedding (training_settings.py: DELTA_VAR, DELTA_DIST, NORM); off at weight 0
    parser.add_argument('--disc-weight', type=float, default=0.0, help='weight of the discriminative embedding loss (0: off)')
    parser.add_argument('--delta-var', type=float, default=0.5, help='pull margin of the discriminative loss')
    parser.add_argument('--delta-dist', type=float, default=1.5, help='push margin of the discriminative loss')
    parser.add_argument('--disc-norm', type=int, default=2, choices=[1, 2], help='norm of the discriminative loss')
    parser.add_argument('--disc-form', default='reference', choices=['reference', 'full'],
                        help="'reference': var + 0.005 qreg on unit means; 'full': var + dist + 0.001 reg")
    # the border term of the cross-entropy (U-Net weight map of the step's instance targets, on the device); off at weight 0
    parser.add_argument('--border-weight', type=float, default=0.0, help='w0 of the border weight map 1 + w0 * '
                        'exp(-(d1 + d2)^2 / (2 sigma^2)) on the cross-entropy of background pixels (0: off)')
    parser.add_argument('--border-sigma', type=float, default=5.0, help='sigma of the border weight map, in pixels')
    parser.add_argument('--class-weights', default=None, help='one weight per class, comma separated (w0,w1,...)')
    parser.add_argument('--optimize-bg', action='store_true', help='Dice over every class, background included')
    parser.add_argument('--n-classes', type=int, default=2, help='semantic classes, 2..32 (more than 2 needs --semantic-only)')
    parser.add_argument('--semantic-only', action='store_true', help='train the semantic network alone (no instance head)')
    # the optimizer (training_settings.py: OPTIMIZER, LEARNING_RATE, WEIGHT_DECAY, TRAIN_CNN); the defaults are the shipped
    # settings.  lr 1.0 is an Adadelta value: Adam and RMSprop want about 1e-3, SGD about 1e-2
    parser.add_argument('--optimizer', default='Adadelta', choices=['Adadelta', 'Adam', 'RMSprop', 'SGD'])
    parser.add_argument('--lr', type=float, default=1.0, help='learning rate [Default: 1.0]')
    parser.add_argument('--weight-decay', type=float, default=0.001, help='L2 weight decay [Default: 0.001]')
    parser.add_argument('--freeze-cnn', action='store_true', help='do not update the backbone (fit\'s train_cnn=False)')
    parser.add_argument('--val-scores', action='store_true', help='also segment and score every validation minibatch: '
                        'per-epoch SBD, |DiC| and FG Dice in <out>/validation_scores.log (Model.val_scores)')
    parser.add_argument('--val-sem-scores', action='store_true', help='also score the semantic prediction of every validation '
                        'minibatch: per-epoch mIoU, pixel accuracy and mean Dice of the epoch-total confusion matrix in '
                        '<out>/validation_sem_scores.log (Model.val_sem_scores)')
    # AlignCollate's five photometric augmentations, which the reference ships disabled (training_settings.py:42-46 COLOR_JITTERING,
    # GAMMA_ADJUSTMENT, CHANNEL_SWAPPING, GRAYSCALING, RESOLUTION_DEGRADING): for the training loader of --data only
    parser.add_argument('--color-jitter', action='store_true', help='random brightness / contrast / saturation / hue')
    parser.add_argument('--gamma', action='store_true', help='random gamma in [0.7, 1.3]')
    parser.add_argument('--channel-swap', action='store_true', help='random channel map, with probability 0.5')
    parser.add_argument('--grayscale', action='store_true', help='grayscale with probability 0.3')
    parser.add_argument('--resolution', action='store_true', help='Lanczos resize by a ratio in [0.7, 1.3] and back')
    # elastic deformation of image and annotation together (not in the reference; RecordLoader(elastic=True)): for the
    # training loader of --data only.  The defaults are a stated choice, not a tuned one
    parser.add_argument('--elastic', action='store_true', help='smooth random elastic deformation, once per batch')
    parser.add_argument('--elastic-alpha', type=float, nargs=2, default=[0.0, 100.0], metavar=('LO', 'HI'),
                        help='the field is alpha * (blurred noise in [-1, 1)), alpha uniform in [LO, HI] per image')
    parser.add_argument('--elastic-sigma', type=float, default=8.0, help='sigma of the Gaussian blur of the field, in pixels')
    parser.add_argument('--elastic-p', type=float, default=0.5, help='probability that an image is deformed')
    # copy-paste of instances between the images of a batch (not in the reference; RecordLoader(copy_paste=True)): for the
    # training loader of --data only.  The defaults are a stated choice, not a tuned one
    parser.add_argument('--copy-paste', action='store_true', help='paste instances of another image of the batch, once per batch')
    parser.add_argument('--copy-paste-p', type=float, default=0.5, help='probability that an image receives a paste')
    parser.add_argument('--copy-paste-min-area', type=int, default=16, help='a pasted instance keeps at least this many pixels')
    parser.add_argument('--copy-paste-shift', type=float, default=0.5,
                        help='the pasted instances move by up to this fraction of the side, in both directions')
    return parser


def parse_args(argv=None):
    parser = build_parser()
    opt = parser.parse_args(argv)
    if opt.dataset not in ['CVPPP', ]:
        parser.error('--dataset must be CVPPP')
    if not 2 <= opt.n_classes <= 32:
        parser.error('--n-classes must be in [2, 32]')
    if opt.n_classes > 2 and not opt.semantic_only:
        parser.error('--n-classes > 2 needs --semantic-only: the instance head reads a foreground / background mask')
    if opt.border_weight < 0 or not opt.border_sigma > 0:
        parser.error('--border-weight must not be negative and --border-sigma must be positive')
    if opt.border_weight > 0 and opt.criterion == 'Lovasz':
        parser.error('--border-weight weighs the cross-entropy: --criterion Lovasz has none (use CELovasz)')
    if not (opt.elastic_alpha[0] <= opt.elastic_alpha[1] and 0.0 <= opt.elastic_p <= 1.0 and 0.0 <= opt.elastic_sigma <= 16.0):
        parser.error('--elastic-alpha LO HI needs LO <= HI, --elastic-p a probability and --elastic-sigma at most 16 '
                     '(a blur radius of 64 pixels)')
    if not (0.0 <= opt.copy_paste_p <= 1.0 and opt.copy_paste_min_area >= 1 and 0.0 <= opt.copy_paste_shift <= 1.0):
        parser.error('--copy-paste-p needs a probability, --copy-paste-min-area at least 1 and --copy-paste-shift a fraction '
                     'in [0, 1]')
    if opt.class_weights is not None:
        try:
            opt.class_weights = [float(v) for v in opt.class_weights.split(',')]
        except ValueError:
            parser.error('--class-weights: comma separated numbers')
        if len(opt.class_weights) != opt.n_classes:
            parser.error('--class-weights: %d values for %d classes' % (len(opt.class_weights), opt.n_classes))
    return opt


def fit_arguments(opt):
    """Model.fit's arguments ahead of the loaders, as the reference's train.py passes them (training_settings.py)."""
    return (opt.criterion, opt.delta_var, opt.delta_dist, opt.disc_norm, opt.lr, opt.weight_decay, 10.0, 0.5, 25, opt.optimize_bg, opt.optimizer,
            not opt.freeze_cnn, opt.nepochs, opt.class_weights)


def fit_keywords(opt):
    """Model.fit's keyword arguments: the discriminative loss and the border term."""
    return dict(disc_weight=opt.disc_weight, disc_form=opt.disc_form, border_weight=opt.border_weight,
                border_sigma=opt.border_sigma)


def photometric_arguments(opt):
    """RecordLoader's photometric flags: the training loader's alone."""
    return dict(color_jitter=opt.color_jitter, gamma=opt.gamma, channel_swap=opt.channel_swap, grayscale=opt.grayscale,
                resolution=opt.resolution)


def elastic_arguments(opt):
    """RecordLoader's elastic-deformation arguments: the training loader's alone."""
    return dict(elastic=opt.elastic, elastic_alpha=tuple(opt.elastic_alpha), elastic_sigma=opt.elastic_sigma,
                elastic_p=opt.elastic_p)


def copy_paste_arguments(opt):
    """RecordLoader's copy-paste arguments: the training loader's alone."""
    return dict(copy_paste=opt.copy_paste, copy_paste_p=opt.copy_paste_p, copy_paste_min_area=opt.copy_paste_min_area,
                copy_paste_shift=opt.copy_paste_shift)


def main(argv=None):
    opt = parse_args(argv)
    import isa_amd  # noqa: F401
    from isa_amd.model import Model
    from isa_amd.data import SyntheticLoader
    from isa_amd import parallel
    world, rank, local_rank = parallel.init_from_env()           # binds the GPU before anything else touches it
    assert opt.batchsize % world == 0, "--batchsize is the global batch: it must divide by the number of ranks"
    per_rank = opt.batchsize // world
    SEED = 23                                                     # training_settings.py:53
    random.seed(parallel.rank_seed(SEED, rank)); np.random.seed(parallel.rank_seed(SEED, rank))
    torch.manual_seed(parallel.rank_seed(SEED, rank))             # instance order, glimpse points, dropout: per rank
    model = Model(opt.dataset, 'ReSeg', opt.n_classes, 32, use_instance_segmentation=not opt.semantic_only,
                  load_model_path=opt.model, usegpu=True, dtype=torch.bfloat16 if opt.dtype == 'bf16' else torch.float32)
    model.val_scores = opt.val_scores
    model.val_sem_scores = opt.val_sem_scores
    model.lovasz_per_image, model.lovasz_only_present = opt.lovasz_per_image, opt.lovasz_present
    # every rank draws its own shard of each global batch (weights start identical: the model seed is not per rank)
    train_loader = SyntheticLoader(opt.iters_per_epoch, per_rank, opt.size, opt.size, seed=parallel.rank_seed(SEED, rank),
                                   compact=opt.compact_targets, n_classes=opt.n_classes)
    test_loader = SyntheticLoader(max(1, opt.iters_per_epoch // 4), per_rank, opt.size, opt.size,
                                  seed=parallel.rank_seed(SEED + 7, rank), compact=opt.compact_targets,
                                  n_classes=opt.n_classes)
    if opt.data:                      # the reference's datasets (train.py:87-147): records -> device-side collate
        from isa_amd.records import RecordDataset, RecordLoader
        train_loader = RecordLoader(RecordDataset(os.path.join(opt.data, 'training-lmdb')), per_rank, opt.size, opt.size,
                                    mode='training', seed=SEED, rank=rank, world=world, **photometric_arguments(opt),
                                    **elastic_arguments(opt), **copy_paste_arguments(opt))
        test_loader = RecordLoader(RecordDataset(os.path.join(opt.data, 'validation-lmdb')), per_rank, opt.size, opt.size,
                                   mode='test', seed=SEED, rank=rank, world=world)
    model.fit(*fit_arguments(opt), train_loader, test_loader, opt.out, opt.debug, **fit_keywords(opt))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
