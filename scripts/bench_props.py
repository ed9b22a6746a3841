#!/usr/bin/env python3
"""Time of measuring instances: the device entries against the host way.

Maps uint8 [16,256,256] and [16,1024,1024], already on the device (where ReSeg.segment leaves them), with 8 and 32 objects:
  "leaves":  elliptical instances on a background that covers most of the image (what a leaf map looks like);
  "uniform": the image cut into as many rectangles, no background (every pixel is accumulated: the worst case).
Timed:
  props   isa_label_props alone (its two launches: set acc to the empty values, accumulate), no image, into
          preallocated buffers: device events around --reps back-to-back calls, the time of one call; the median of
          --calls such windows taken in turn with the other variants.  bytes / time is the MAP's bytes (n*h*w, what has
          to be read at least) over that time.
  rgb     the same with the uint8 RGB image [n,h,w,3] (its bytes are read under labelled pixels only).
  e2e     ReSeg.instance_properties(labels, check=False): allocation, isa_label_props, isa_instance_props; host clock
          around a device synchronise, median of --calls.
  host    the host way: labels.cpu(), then per image scipy.ndimage.find_objects / sum_labels / center_of_mass (area, box,
          centroid only - no second moments, no perimeter); median of --host-calls.
Needs a GPU; there is no fallback.  Writes its lines to --out."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import isa_amd  # noqa: F401,E402
import props_np as P  # noqa: E402
from isa_amd import lib as L  # noqa: E402
from isa_amd.labelmaps import LabelOps  # noqa: E402
from scipy import ndimage  # noqa: E402


def make_maps(kind, B, size, k, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    m = np.zeros((B, size, size), np.uint8)
    if kind == "uniform":
        cols = int(np.ceil(np.sqrt(k)))
        rows = (k + cols - 1) // cols
        m[:] = (np.minimum(yy * rows // size, rows - 1) * cols + np.minimum(xx * cols // size, cols - 1)) % k + 1
        return m
    for b in range(B):
        for v in range(k):
            cy, cx = rng.uniform(0.1, 0.9, 2) * size
            ry, rx = rng.uniform(0.03, 0.08, 2) * size * (8.0 / k) ** 0.5
            inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            m[b][inside & (m[b] == 0)] = v + 1
    return m


def host_props(labels, k):
    lab = labels.cpu().numpy()
    out = []
    index = list(range(1, k + 1))
    for img in lab:
        ones = np.ones_like(img, dtype=np.float64)
        out.append((ndimage.find_objects(img.astype(np.int32), max_label=k), ndimage.sum_labels(ones, img, index),
                    ndimage.center_of_mass(ones, img, index)))
    return out


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--objects", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "props_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_props.py needs the GPU"
    B = opt.batch
    lib = L.checked()
    lines = ["props bench: %s, maps uint8 [%d,S,S]; props / rgb: device events around %d back-to-back isa_label_props calls, "
             "per call, median of %d windows taken in turn; e2e: host clock around a device synchronise, median of %d; host: "
             "labels.cpu() + scipy.ndimage find_objects / sum_labels / center_of_mass per image, median of %d"
             % (torch.cuda.get_device_name(0), B, opt.reps, opt.calls, opt.calls, opt.host_calls)]
    m = LabelOps()
    for size in opt.sizes:
        rgb = torch.randint(0, 256, (B, size, size, 3), dtype=torch.uint8, device="cuda")
        for k in opt.objects:
            for kind in ("leaves", "uniform"):
                maps_np = make_maps(kind, B, size, k, seed=size + k)
                maps = torch.from_numpy(maps_np).cuda()
                acc = torch.empty((B, 256, L.PROPS_ACC), dtype=torch.int64, device="cuda")
                oob = torch.empty((B,), dtype=torch.int32, device="cuda")
                st = L.stream_ptr()
                variants = {"props": lambda: lib.isa_label_props(maps, None, B, size, size, 0, 256, acc, oob, st),
                            "rgb": lambda: lib.isa_label_props(maps, rgb, B, size, size, 3, 256, acc, oob, st)}
                variants["props"]()
                want = P.label_props(maps_np[:1], None, 256)[0]
                assert np.array_equal(acc[:1].cpu().numpy(), want), "the device result differs from the restatement"
                e2e = lambda: m.instance_properties(maps, check=False)
                for fn in list(variants.values()) + [e2e]:               # warm-up: allocator, code objects
                    fn()
                ms = {name: [] for name in list(variants) + ["e2e"]}
                for _ in range(opt.calls):
                    for name, fn in variants.items():
                        ms[name].append(event_ms(fn, opt.reps))
                    ms["e2e"].append(timed_ms(e2e))
                host = statistics.median(timed_ms(lambda: host_props(maps, k)) for _ in range(opt.host_calls))
                t = {name: statistics.median(v) for name, v in ms.items()}
                fg = float((maps_np != 0).mean())
                gbs = B * size * size / (t["props"] * 1e-3) / 1e9
                lines.append("S %4d  %2d objects  %-7s (%4.1f %% labelled)  props %7.4f ms (%7.1f GB/s of map)  rgb %7.4f ms  "
                             "e2e %7.3f ms  host %9.2f ms  host / e2e %7.1f"
                             % (size, k, kind, 100 * fg, t["props"], gbs, t["rgb"], t["e2e"], host, host / t["e2e"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
