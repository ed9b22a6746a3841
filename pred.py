#!/usr/bin/env python3
"""pred.py — the reference's single-image entry point (code/pred.py:12-22,45-50,110-123): image path in, palette PNG
out.  Per lib/prediction.py:33-50,116-124: read RGB, resize to 256x256 (bilinear), ImageEx + standardization (on the
device: isa_image_ex), semantic forward, probability of class 1 up-sampled to the original size with the
cv2.INTER_NEAREST index rule, `> 0.5` -> x255 -> float32 image -> `.convert('P')` -> <name>-fg_mask.png.
softmax(l)[1] > 0.5 is l1 > l0, i.e. the arg-max map the library already returns (isa_chan_argmax), so no probability
map is materialised.  `--synthetic` predicts one random image when no file is at hand (nothing ships with the repo).
`--instances` builds the instance model and also writes <name>-ins_mask.png, <name>-ins_mask_color.png and
<name>-n_objects.npy as pred_list.py --instances does (ReSeg.segment, at most `--max-objects` instances).
`--n-classes K` (K > 2) loads a K-class semantic-only model and also writes <name>-sem_mask.png and
<name>-sem_mask_color.png as pred_list.py --n-classes does (ReSeg.class_map); -fg_mask.png is then class != 0.
`--min-area`, `--keep`, `--connectivity` and `--components` are pred_list.py's: the clean-up of the `--instances` label
map on the device, and the instance files from the connected components of the class map without an instance head.
`--fill [--fill-max-dist D]` is pred_list.py's too: unlabelled foreground goes to the nearest instance after the clean-up.
The reference's hard-coded checkpoint and image paths (pred.py:25-26,112) are flags here."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import isa_amd  # noqa: F401,E402
from isa_amd.model import Model  # noqa: E402
from pred_list import (H, W, add_cleanup_arguments, add_embedding_arguments, add_fill_arguments,  # noqa: E402
                       add_measure_arguments, check_cleanup_arguments, check_embedding_arguments, check_fill_arguments,
                       check_measure_arguments, clean_and_fill, cleanup_arguments, fill_arguments, nearest_upsample,
                       select_and_measure, select_arguments, write_classes, write_instances, write_polygons,
                       write_properties)


def predict_file(model, image, out_dir, name, instances=False, max_objects=32, clean=None, components=None,
                 instances_from='attention', bandwidth=None, fill=None, select=None, properties=False, polygons=None):
    """image: uint8 RGB [h0,w0,3].  Returns the path of the written mask.  clean: ReSeg.clean_instances' keywords for the
    instance map; components: ReSeg.split_components' keywords - the instance files come from the class map's components;
    instances_from='embedding': the instances are mean-shift clusters of the embedding (ReSeg.segment_embedding); fill:
    ReSeg.fill_instances' keywords - unlabelled foreground goes to the nearest instance after the clean-up; select:
    ReSeg.select_instances' keywords - the instances are then filtered and renumbered by their measurements; properties:
    also write <name>-instances.csv and <name>-ins_mask_model.png (pred_list.write_properties); polygons: ReSeg.polygons'
    keywords - also write <name>-polygons.json (pred_list.write_polygons)."""
    from PIL import Image
    from isa_amd.data import resize_bilinear
    x = resize_bilinear(torch.from_numpy(image[None]), (H, W))  # uint8 [1,H,W,3] on the device, bit-identical to PIL's
                                                               # BILINEAR resize (prediction.py:37); ImageEx follows there
    net = model.model
    net.eval()
    labels = classes = props = polys = None
    with torch.no_grad():
        if net.n_classes > 2:
            net(False, x)
            classes = net.class_map()
            if components is not None:
                labels, counts, _ = net.split_components(classes, **components)
            classes = classes[0].cpu().numpy()                 # uint8 [H,W]: the arg-max taken on the device
            sem_arg = torch.from_numpy((classes != 0).astype(np.float32))[None, None]
        elif instances:
            if instances_from == 'embedding':
                _, sem_arg, labels, counts = net.segment_embedding(x, max_objects=min(max_objects, 32), bandwidth=bandwidth)
            else:
                _, sem_arg, labels, counts = net.segment(x, max_objects)
            # at model resolution, before the nearest up-sampling
            labels, counts = clean_and_fill(net, labels, counts, clean, fill)
        else:
            _, sem_arg = net(False, x)                         # arg-max map == (softmax[:, 1] > 0.5)
            if components is not None:
                labels, counts, _ = net.split_components(net.class_map(), **components)
        if labels is not None:
            labels, counts, props = select_and_measure(net, labels, counts, x, select, properties)
            if polygons is not None:
                polys = net.polygons(labels, **polygons)
    fg = sem_arg[0, 0].cpu().numpy() > 0.5
    full = nearest_upsample(fg, image.shape[0], image.shape[1])            # prediction.py:47-50
    fg_seg_pred_norm = (full * 255).astype(np.float32)                     # pred.py:117
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, name + '-fg_mask.png')
    Image.fromarray(fg_seg_pred_norm).convert('P').save(path)              # pred.py:122-123
    if classes is not None:
        write_classes(out_dir, name, classes, image.shape[0], image.shape[1])
    if labels is not None:
        write_instances(out_dir, name, labels[0].cpu().numpy(), int(counts[0]), image.shape[0], image.shape[1])
    if props is not None:
        write_properties(out_dir, name, labels[0].cpu().numpy(), props[0].cpu().numpy(), int(counts[0]), image.shape[0],
                         image.shape[1])
    if polys is not None:
        write_polygons(out_dir, name, labels[0].cpu().numpy(), polys[0], image.shape[0], image.shape[1])
    return path


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--image', default='', help='Path of the image')
    parser.add_argument('--model', default='', help='Path of the model (state_dict .pth)')
    parser.add_argument('--usegpu', action='store_true', help='kept for flag compatibility: the HIP path is the only path')
    parser.add_argument('--output', default=os.path.join(ROOT, 'outputs'), help='Path of the output directory')
    parser.add_argument('--n_workers', type=int, default=1, help='accepted for compatibility')
    parser.add_argument('--dataset', type=str, default='CVPPP')
    parser.add_argument('--synthetic', action='store_true', help='predict one random 530x500 image instead of --image')
    parser.add_argument('--instances', action='store_true', help='also write -ins_mask.png, -ins_mask_color.png, -n_objects.npy')
    parser.add_argument('--max-objects', type=int, default=32, help='most instances with --instances (1..255)')
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


def main():
    opt = parse_args()
    assert opt.dataset in ['CVPPP', ]                          # pred.py:29
    assert opt.image or opt.synthetic, "give --image or --synthetic"
    if opt.synthetic:
        image, name = np.random.default_rng(0).integers(0, 256, (530, 500, 3), dtype=np.uint8), 'synthetic'
    else:
        from PIL import Image
        assert os.path.isfile(opt.image), 'Image : {} does not exists!'.format(opt.image)
        image, name = np.asarray(Image.open(opt.image).convert('RGB')), os.path.splitext(os.path.basename(opt.image))[0]
    model = Model(opt.dataset, 'ReSeg', opt.n_classes, 32, use_instance_segmentation=opt.instances,
                  load_model_path=opt.model, usegpu=True)
    components = {'connectivity': opt.connectivity, 'min_area': opt.min_area, 'max_objects': opt.max_objects} \
        if opt.components else None
    path = predict_file(model, image, opt.output, name, opt.instances, opt.max_objects, cleanup_arguments(opt), components,
                        opt.instances_from, opt.bandwidth, fill_arguments(opt), select_arguments(opt), opt.properties,
                        {'connectivity': opt.connectivity} if opt.polygons else None)
    print('wrote', path)


if __name__ == '__main__':
    main()
