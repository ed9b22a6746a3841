#!/usr/bin/env python3
"""pred_list.py — batched foreground prediction over a list of images, the working part of the reference's
code/pred_list.py:16-99 (flags --lst/--model/--usegpu/--dataset; outputs <name>.png and <name>-fg_mask.png under
outputs/<dataset>/<model dir>-<model name>/<subset>/).

Per image (lib/prediction.py:33-50,116-124): read RGB, resize to 256x256 (bilinear, `image_resizer`), ImageEx +
standardization (on the device here: isa_image_ex), network forward, softmax > 0.5 (= the arg-max map), nearest-neighbour up-sampling
to the original size (cv2.INTER_NEAREST index rule), x255, PNG.
`--instances` builds the instance model and also writes the reference's instance outputs (pred_list.py:88-99), the
files evaluate.py reads: <name>-ins_mask.png (uint8 label map, 0 = no instance, brought to the original size by the
same nearest-neighbour rule), <name>-ins_mask_color.png (the labels through a fixed palette) and <name>-n_objects.npy.
The reference fills them from `Prediction.cluster`, which is dead at HEAD (its GT-free instance path
raises UnboundLocalError, reseg.py:126); here they come from ReSeg.segment - one glimpse point and one decoder pass per
object, at most `--max-objects` per image.  Without the flag nothing but the two foreground files is written.
`--n-classes K` (K > 2) loads a K-class semantic-only model and also writes <name>-sem_mask.png (uint8 class ids at the
original size, same nearest-neighbour rule) and <name>-sem_mask_color.png (the ids through the palette); -fg_mask.png is
then (class != 0) * 255.  The class map is taken on the device from the logits (ReSeg.class_map): no softmax comes down.
`--instances-from embedding` takes the `--instances` label maps from mean-shift clustering of the instance embedding
(ReSeg.segment_embedding; `--bandwidth` sets the ball's radius) instead of the attention decoder; the files are the same.
`--min-area N`, `--keep largest|all` and `--connectivity 4|8` clean the `--instances` label maps on the device, at model
resolution and before the up-sampling (ReSeg.clean_instances: the largest connected piece of every instance, or every
piece as an object of its own; pieces under N pixels dropped).  `--components` needs no instance head: the connected
components of the predicted class map (ReSeg.split_components; `--min-area`, `--connectivity`, `--max-objects` apply) are
written as <name>-ins_mask.png, <name>-ins_mask_color.png and <name>-n_objects.npy - the count-the-blobs baseline.
`--fill` gives, after that clean-up, every foreground pixel of the predicted class map that no instance holds to the
nearest instance (ReSeg.fill_instances, on the device); `--fill-max-dist D` only within D pixels.
`--order label|area|raster`, `--clear-border` and `--max-area N` then filter and renumber the instances of `--instances` or
`--components` by their measurements (ReSeg.select_instances: largest first, truncated objects dropped); `--properties`
measures what is left on the device (ReSeg.instance_properties) and writes <name>-instances.csv - one row per instance in
the columns reseg.PROPS_COLUMNS, taken at model resolution, followed by model_w, model_h, orig_w, orig_h so that a caller
can rescale - and <name>-ins_mask_model.png, the label map at model resolution that the rows describe.
`--polygons` traces the outlines of what is left on the device (ReSeg.polygons, under `--connectivity`) and writes
<name>-polygons.json: model_w, model_h, orig_w, orig_h and one {label, outer, holes} entry per connected piece, rings of
[x, y] pixel corners at model resolution; <name>-ins_mask_model.png is written with it.
`--synthetic N` runs N random images instead of a list (no files needed)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import isa_amd  # noqa: F401,E402
from isa_amd.model import Model  # noqa: E402
from isa_amd.data import resize_bilinear  # noqa: E402

H = W = 256                                             # data_settings.py: IMAGE_HEIGHT / IMAGE_WIDTH


def nearest_upsample(mask, out_h, out_w):
    """cv2.resize(..., interpolation=cv2.INTER_NEAREST): src = min(floor(dst * scale), size - 1)."""
    h, w = mask.shape
    ys = np.minimum((np.arange(out_h) * (h / out_h)).astype(np.int64), h - 1)
    xs = np.minimum((np.arange(out_w) * (w / out_w)).astype(np.int64), w - 1)
    return mask[ys][:, xs]


def label_palette():
    """256 fixed RGB colours for label maps: 0 is black, the others are spread by a multiplicative hash so that
    neighbouring labels differ clearly.  No plotting library."""
    k = np.arange(256, dtype=np.uint32)
    pal = np.stack([(k * 97 + 59) % 200 + 56, (k * 173 + 101) % 200 + 56, (k * 41 + 7) % 200 + 56], 1).astype(np.uint8)
    pal[0] = 0
    return pal


def write_instances(d, name, labels, n_objects, out_h, out_w):
    """The reference's three instance files for one image (pred_list.py:91-99).  labels: uint8 [h,w]."""
    from PIL import Image
    full = nearest_upsample(labels, out_h, out_w).astype(np.uint8)
    Image.fromarray(full).save(os.path.join(d, name + '-ins_mask.png'))
    Image.fromarray(label_palette()[full]).save(os.path.join(d, name + '-ins_mask_color.png'))
    np.save(os.path.join(d, name + '-n_objects.npy'), np.int64(n_objects))


def write_classes(d, name, classes, out_h, out_w):
    """The two class-map files of one image of a K-class model.  classes: uint8 [h,w].  Returns the full-size map."""
    from PIL import Image
    full = nearest_upsample(classes, out_h, out_w).astype(np.uint8)
    Image.fromarray(full).save(os.path.join(d, name + '-sem_mask.png'))
    Image.fromarray(label_palette()[full]).save(os.path.join(d, name + '-sem_mask_color.png'))
    return full


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--lst', default='', help='Text file that contains image paths')
    parser.add_argument('--model', default='', help='Path of the model (state_dict .pth)')
    parser.add_argument('--usegpu', action='store_true', help='kept for flag compatibility: the HIP path is the only path')
    parser.add_argument('--dataset', type=str, default='CVPPP')
    parser.add_argument('--output', default='', help='output directory (default: the reference layout under outputs/)')
    parser.add_argument('--batch', type=int, default=16)
    parser.add_argument('--synthetic', type=int, default=0, help='predict N random images instead of --lst')
    parser.add_argument('--instances', action='store_true', help='also write -ins_mask.png, -ins_mask_color.png, -n_objects.npy')
    parser.add_argument('--max-objects', type=int, default=32, help='most instances per image with --instances (1..255)')
    parser.add_argument('--n-classes', type=int, default=2, help='semantic classes of the model, 2..32; more than 2: a '
                        'semantic-only model, also writes -sem_mask.png and -sem_mask_color.png')
    add_cleanup_arguments(parser)
    add_embedding_arguments(parser)
    add_fill_arguments(parser)
    add_measure_arguments(parser)
    opt = parser.parse_args(argv)
    if not 2 <= opt.n_classes <= 32:
        parser.error('--n-classes must be in [2, 32]')
    if opt.n_classes > 2 and opt.instances:
        parser.error('--instances needs the 2-class model: a K-class network is semantic-only')
    check_cleanup_arguments(parser, opt)
    check_embedding_arguments(parser, opt)
    check_fill_arguments(parser, opt)
    check_measure_arguments(parser, opt)
    return opt


def add_embedding_arguments(parser):
    parser.add_argument('--instances-from', choices=['attention', 'embedding'], default='attention', help='with '
                        '--instances: the attention decoder (ReSeg.segment) or mean-shift clustering of the instance '
                        'embedding (ReSeg.segment_embedding: no decoder pass, at most 32 instances)')
    parser.add_argument('--bandwidth', type=float, default=None, help='with --instances-from embedding: the radius of the '
                        'mean-shift ball (default: delta_dist = 1.5)')


def check_embedding_arguments(parser, opt):
    if opt.instances_from != 'attention' and not opt.instances:
        parser.error('--instances-from chooses where the instances of --instances come from')
    if opt.bandwidth is not None and opt.instances_from != 'embedding':
        parser.error('--bandwidth needs --instances-from embedding')
    if opt.bandwidth is not None and not opt.bandwidth > 0:
        parser.error('--bandwidth must be positive')


def segment_instances(net, x, opt):
    """(sem_argmax, labels, n_objects) of the --instances label maps: ReSeg.segment, or ReSeg.segment_embedding."""
    if opt.instances_from == 'embedding':
        _, sem_arg, labels, counts = net.segment_embedding(x, max_objects=min(opt.max_objects, 32),
                                                           bandwidth=opt.bandwidth)
    else:
        _, sem_arg, labels, counts = net.segment(x, opt.max_objects)
    return sem_arg, labels, counts


def add_cleanup_arguments(parser):
    parser.add_argument('--min-area', type=int, default=0, help='with --instances or --components: drop connected pieces '
                        'under N pixels (at model resolution)')
    parser.add_argument('--keep', choices=['largest', 'all'], default=None, help='with --instances: keep the largest '
                        'connected piece of every instance, or make every piece an instance of its own')
    parser.add_argument('--connectivity', type=int, choices=[4, 8], default=8, help='neighbourhood of the connected pieces')
    parser.add_argument('--components', action='store_true', help='write -ins_mask.png, -ins_mask_color.png and '
                        '-n_objects.npy from the connected components of the predicted class map (no instance head)')


def check_cleanup_arguments(parser, opt):
    if opt.components and opt.instances:
        parser.error('--components and --instances both write the -ins_mask files: give one of them')
    if opt.keep is not None and not opt.instances:
        parser.error('--keep cleans the instances of --instances')
    if opt.min_area > 1 and not (opt.instances or opt.components):
        parser.error('--min-area needs --instances or --components')


def add_fill_arguments(parser):
    parser.add_argument('--fill', action='store_true', help='with --instances: after the clean-up, give every foreground '
                        'pixel without an instance to the nearest instance')
    parser.add_argument('--fill-max-dist', type=float, default=None, help='with --fill: only within this many pixels')


def check_fill_arguments(parser, opt):
    if opt.fill and not opt.instances:
        parser.error('--fill fills the instances of --instances')
    if opt.fill_max_dist is not None and not opt.fill:
        parser.error('--fill-max-dist needs --fill')
    if opt.fill_max_dist is not None and opt.fill_max_dist < 0:
        parser.error('--fill-max-dist must not be negative')


def fill_arguments(opt):
    """ReSeg.fill_instances' keywords for the --instances label maps, or None without --fill."""
    return {'max_dist': opt.fill_max_dist} if opt.fill else None


def clean_and_fill(net, labels, counts, clean, fill):
    """The --instances label maps after the clean-up (ReSeg.clean_instances' keywords, or None) and the fill against the
    foreground of the predicted class map (ReSeg.fill_instances' keywords, or None): at model resolution, on the device."""
    if clean is not None:
        labels, counts, _ = net.clean_instances(labels, **clean)
    if fill is not None:
        labels, _ = net.fill_instances(labels, net.class_map(), **fill)
    return labels, counts


def add_measure_arguments(parser):
    parser.add_argument('--properties', action='store_true', help='with --instances or --components: measure every instance '
                        'on the device (ReSeg.instance_properties) and write <name>-instances.csv, one row per instance, '
                        'and <name>-ins_mask_model.png, the label map at model resolution that the rows describe')
    parser.add_argument('--polygons', action='store_true', help='with --instances or --components: trace every instance on '
                        'the device (ReSeg.polygons) and write <name>-polygons.json, outer rings and holes as [x, y] pixel '
                        'corners at model resolution, and <name>-ins_mask_model.png')
    parser.add_argument('--order', choices=['label', 'area', 'raster'], default=None, help='with --instances or '
                        '--components: renumber the instances by old label, largest first, or by first pixel')
    parser.add_argument('--clear-border', action='store_true', help='with --instances or --components: drop the instances '
                        'that touch the image edge')
    parser.add_argument('--max-area', type=int, default=None, help='with --instances or --components: drop the instances '
                        'of more than N pixels (at model resolution)')


def check_measure_arguments(parser, opt):
    if (opt.properties or opt.order or opt.clear_border or opt.max_area is not None) and not (opt.instances or opt.components):
        parser.error('--properties, --order, --clear-border and --max-area need --instances or --components')
    if opt.polygons and not (opt.instances or opt.components):
        parser.error('--polygons needs --instances or --components')
    if opt.max_area is not None and opt.max_area < 1:
        parser.error('--max-area must be positive')


def select_arguments(opt):
    """ReSeg.select_instances' keywords for the label maps, or None when the flags ask for no selection."""
    if opt.order is None and not opt.clear_border and opt.max_area is None:
        return None
    return {'order': opt.order or 'label', 'clear_border': opt.clear_border, 'max_area': opt.max_area,
            'max_objects': opt.max_objects}


def select_and_measure(net, labels, counts, x, select, properties):
    """The label maps after the selection by measurement (ReSeg.select_instances' keywords, or None), and with `properties`
    the measurements of what is left (ReSeg.instance_properties with the colour means of the uint8 RGB batch x), else
    None: at model resolution, on the device."""
    if select is not None:
        labels, counts, _ = net.select_instances(labels, **select)
    return labels, counts, (net.instance_properties(labels, x) if properties else None)


def write_properties(d, name, labels, props, n_objects, out_h, out_w):
    """<name>-instances.csv: the columns reseg.PROPS_COLUMNS of instances 1..n_objects (row k: label k), measured at model
    resolution, then both sizes so that a caller can rescale; <name>-ins_mask_model.png: the uint8 label map [h,w] the
    rows describe."""
    from PIL import Image
    from isa_amd.reseg import PROPS_COLUMNS
    h, w = labels.shape
    sizes = ['%d' % v for v in (w, h, out_w, out_h)]
    with open(os.path.join(d, name + '-instances.csv'), 'w') as f:
        f.write(','.join(PROPS_COLUMNS + ('model_w', 'model_h', 'orig_w', 'orig_h')) + '\n')
        for k in range(1, int(n_objects) + 1):
            f.write(','.join([repr(float(v)) for v in props[k]] + sizes) + '\n')
    Image.fromarray(labels).save(os.path.join(d, name + '-ins_mask_model.png'))


def write_polygons(d, name, labels, polys, out_h, out_w):
    """<name>-polygons.json: the sizes, as in the properties CSV, and ReSeg.polygons' entries of one image with the rings as
    lists of [x, y] at model resolution; <name>-ins_mask_model.png: the uint8 label map [h,w] they outline."""
    import json
    from PIL import Image
    h, w = labels.shape
    doc = {'model_w': w, 'model_h': h, 'orig_w': int(out_w), 'orig_h': int(out_h),
           'polygons': [{'label': p['label'], 'outer': p['outer'].tolist(), 'holes': [r.tolist() for r in p['holes']]}
                        for p in polys]}
    with open(os.path.join(d, name + '-polygons.json'), 'w') as f:
        json.dump(doc, f)
    Image.fromarray(labels).save(os.path.join(d, name + '-ins_mask_model.png'))


def cleanup_arguments(opt):
    """ReSeg.clean_instances' keywords for the --instances label maps, or None when the flags ask for no clean-up."""
    if opt.keep is None and opt.min_area <= 1:
        return None
    return {'keep': opt.keep or 'all', 'connectivity': opt.connectivity, 'min_area': opt.min_area,
            'max_objects': opt.max_objects}


def main():
    opt = parse_args()
    assert opt.dataset in ['CVPPP', ]                    # pred_list.py:26
    assert opt.lst or opt.synthetic, "give --lst or --synthetic N"

    if opt.synthetic:
        rng = np.random.default_rng(0)
        names = ['synthetic_%04d' % i for i in range(opt.synthetic)]
        loaders = [lambda i=i: rng.integers(0, 256, (300 + 7 * (i % 5), 330, 3), dtype=np.uint8) for i in range(opt.synthetic)]
        subset, tag = 'synthetic', 'random'
    else:
        from PIL import Image
        paths = [str(p) for p in np.atleast_1d(np.loadtxt(opt.lst, dtype='str', delimiter=','))]
        names = [os.path.splitext(os.path.basename(p))[0] for p in paths]
        loaders = [lambda p=p: np.asarray(Image.open(p).convert('RGB')) for p in paths]
        subset = os.path.basename(opt.lst).split('_')[0]
        tag = (os.path.basename(os.path.dirname(opt.model)) + '-' + os.path.splitext(os.path.basename(opt.model))[0]) \
            if opt.model else 'random'
    out_dir = opt.output or os.path.join(ROOT, 'outputs', opt.dataset, tag, subset)
    os.makedirs(out_dir, exist_ok=True)

    from PIL import Image
    model = Model(opt.dataset, 'ReSeg', opt.n_classes, 32, use_instance_segmentation=opt.instances,
                  load_model_path=opt.model, usegpu=True)
    net = model.model
    net.eval()
    done = 0
    for s in range(0, len(names), opt.batch):
        imgs = [ld() for ld in loaders[s:s + opt.batch]]
        # resize on the device (isa_resize_bilinear_u8, bit-identical to PIL's BILINEAR): one launch per source size
        x = torch.cat([resize_bilinear(torch.from_numpy(im[None]), (H, W)) for im in imgs])   # uint8 [B,H,W,3]; ImageEx follows
        labels = counts = classes = props = polys = None
        select = select_arguments(opt)
        if opt.n_classes > 2:
            with torch.no_grad():
                net(False, x)
                classes = net.class_map()                # uint8 [B,H,W] on the device: one byte per pixel comes down
            sem_arg = (classes != 0).to(torch.float32)[:, None]
            if opt.components:
                labels, counts, _ = net.split_components(classes, connectivity=opt.connectivity, min_area=opt.min_area,
                                                         max_objects=opt.max_objects)
                labels, counts, props = select_and_measure(net, labels, counts, x, select, opt.properties)
                polys = net.polygons(labels, connectivity=opt.connectivity) if opt.polygons else None
                labels, counts = labels.cpu().numpy(), counts.cpu().numpy()
            classes = classes.cpu().numpy()
        elif opt.instances:
            sem_arg, labels, counts = segment_instances(net, x, opt)
            # at model resolution, before the nearest up-sampling
            labels, counts = clean_and_fill(net, labels, counts, cleanup_arguments(opt), fill_arguments(opt))
            labels, counts, props = select_and_measure(net, labels, counts, x, select, opt.properties)
            polys = net.polygons(labels, connectivity=opt.connectivity) if opt.polygons else None
            labels, counts = labels.cpu().numpy(), counts.cpu().numpy()
        elif opt.components:
            with torch.no_grad():
                _, sem_arg = net(False, x)
                labels, counts, _ = net.split_components(net.class_map(), connectivity=opt.connectivity,
                                                         min_area=opt.min_area, max_objects=opt.max_objects)
                labels, counts, props = select_and_measure(net, labels, counts, x, select, opt.properties)
                polys = net.polygons(labels, connectivity=opt.connectivity) if opt.polygons else None
            labels, counts = labels.cpu().numpy(), counts.cpu().numpy()
        else:
            _, sem_arg = net.infer_graphed(x) if len(imgs) == opt.batch else net(False, x)
        # softmax(l)[1] > 0.5 (pred.py:117-121) is l1 > l0: the arg-max map the library already returns
        fg = (sem_arg[:, 0] > 0.5).to(torch.uint8).cpu().numpy()
        props = None if props is None else props.cpu().numpy()
        for i, (im, name, m) in enumerate(zip(imgs, names[s:s + opt.batch], fg)):
            d = os.path.join(out_dir, name)
            os.makedirs(d, exist_ok=True)
            full = nearest_upsample(m, im.shape[0], im.shape[1]) * 255
            Image.fromarray(im).save(os.path.join(d, name + '.png'))
            Image.fromarray(full.astype(np.uint8)).save(os.path.join(d, name + '-fg_mask.png'))
            if labels is not None:
                write_instances(d, name, labels[i], counts[i], im.shape[0], im.shape[1])
            if props is not None:
                write_properties(d, name, labels[i], props[i], counts[i], im.shape[0], im.shape[1])
            if polys is not None:
                write_polygons(d, name, labels[i], polys[i], im.shape[0], im.shape[1])
            if classes is not None:
                write_classes(d, name, classes[i], im.shape[0], im.shape[1])
            done += 1
    print('wrote %d predictions under %s' % (done, out_dir))


if __name__ == '__main__':
    main()
