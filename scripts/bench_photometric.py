#!/usr/bin/env python3
"""One sample's photometric chain - resolution jitter (Lanczos there and back), then colour jitter, gamma, channel swap
and grayscale as one isa_photometric_u8 pass - on the device vs the same chain in Pillow on the host (what the
reference's AlignCollate does per image), at a CVPPP A1 original (530 x 500) and at the largest original (2362 x 672).
python scripts/bench_photometric.py"""
import os, sys, time
import numpy as np
import torch
from PIL import Image
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import isa_amd  # noqa: F401
from isa_amd import data as D
import photometric_np as P

rng = np.random.default_rng(0)
OPS = [("saturation", 1.31), ("hue", -0.11), ("contrast", 0.77), ("brightness", 1.22)]
GAMMA, CHAN, GRAY, RATIO = 0.91, (2, 2, 0), True, 0.85
for h, w in ((530, 500), (672, 2362)):
    x = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    d = torch.from_numpy(x[None]).cuda()
    prog = [D.photo_program(OPS, D.gamma_lut(GAMMA), CHAN, GRAY)]

    def chain():
        return D.photometric(D.resolution_degrade(d, RATIO), prog)

    def pixelwise():
        return D.photometric(d, prog)

    times = []
    for f in (chain, pixelwise):
        for _ in range(3): f()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(20): out = f()
        torch.cuda.synchronize(); times.append((time.perf_counter() - t0) / 20)
    pil = Image.fromarray(x)
    host = []
    for f in (lambda: P.pil_photometric(P.pil_resolution(pil, RATIO), OPS, GAMMA, CHAN, GRAY),
              lambda: P.pil_photometric(pil, OPS, GAMMA, CHAN, GRAY)):
        f(); t0 = time.perf_counter()
        for _ in range(3): ref = f()
        host.append((time.perf_counter() - t0) / 3)
    assert np.array_equal(out[0].cpu().numpy(), np.asarray(ref))
    assert np.array_equal(chain()[0].cpu().numpy(), np.asarray(P.pil_photometric(P.pil_resolution(pil, RATIO), OPS, GAMMA, CHAN, GRAY)))
    print("%4d x %4d  resolution + jitter + gamma + swap + gray: device %7.1f us, Pillow on one host core %7.2f ms;  "
          "the four pixel-wise stages alone: device %7.1f us, Pillow %7.2f ms" %
          (h, w, times[0] * 1e6, host[0] * 1e3, times[1] * 1e6, host[1] * 1e3))
