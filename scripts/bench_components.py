#!/usr/bin/env python3
"""Time of labelling connected components and cleaning instance maps: the device entries against the host way.

Maps uint8 [16,256,256], already on the device (where ReSeg.segment leaves them), at connectivity 4 and 8:
  "blobs": 8 elliptical instances per image with speckles of other labels in them (what segment() leaves behind);
  "noise": binary noise of density 0.59 (the site-percolation threshold of the 4-connected lattice: huge winding
           components, the worst case of the union-find).
Timed, each as the median of --calls calls taken in turn (one call of every variant per round), host clock around a
device synchronise:
  label   isa_cc_label alone (LabelOps.cc_label);
  clean   ReSeg.clean_instances(keep='largest'): isa_cc_label + isa_cc_select(ISA_CC_LARGEST);
  host    the same clean-up the host way: labels.cpu(), scipy.ndimage.label per value when scipy can be imported (else the
          restatement tests/components_np.py), the largest piece of every value, and the copy back; median of --host-calls.
and one ReSeg.segment call at 8 objects on the same batch shape, so that the share of the clean-up can be read off.
The launch counts are those the header states for the shape (they do not depend on the contents).
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
import components_np as cnp  # noqa: E402
import reseg_ref as R  # noqa: E402
from isa_amd import lib as L  # noqa: E402
from isa_amd.reseg import ReSeg  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None


def make_maps(kind, B, size, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return (rng.random((B, size, size)) < 0.59).astype(np.uint8)
    yy, xx = np.mgrid[0:size, 0:size]
    m = np.zeros((B, size, size), np.uint8)
    for b in range(B):
        for k in range(8):
            cy, cx = rng.uniform(0.15, 0.85, 2) * size
            ry, rx = rng.uniform(0.05, 0.14, 2) * size
            inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            m[b][inside & (m[b] == 0)] = k + 1
    speck = (rng.random(m.shape) < 0.03) & (m != 0)
    m[speck] = rng.integers(1, 9, m.shape)[speck]
    return m


def host_clean(labels, conn):
    """clean_instances(keep='largest') on the host: the copy down, the labelling, the selection, the copy back."""
    lab = labels.cpu().numpy()
    if ndimage is None:
        out, count, _ = cnp.largest(lab, cnp.label(lab, conn)[0], 1, 255)
    else:
        structure = ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)
        out, count = np.zeros_like(lab), np.zeros(len(lab), np.int32)
        for b, img in enumerate(lab):
            for v in np.unique(img[img > 0]):
                pieces, k = ndimage.label(img == v, structure)
                area = np.bincount(pieces.reshape(-1))[1:]
                count[b] += 1
                out[b][pieces == 1 + int(np.argmax(area))] = count[b]        # argmax: the first of equal areas
    return torch.from_numpy(out).cuda(), torch.from_numpy(count).cuda()


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_components.py needs the GPU"
    B, size = opt.batch, opt.size
    merge = 1 if size > min(L.CC_TILE_H, L.CC_TILE_W) else 0
    n_label, n_clean = 2 + merge, 2 + merge + 5
    lines = ["components bench: %s, maps uint8 [%d,%d,%d]; median of %d calls taken in turn, host clock around a device "
             "synchronise; host: %s, median of %d calls" % (torch.cuda.get_device_name(0), B, size, size, opt.calls,
                                                            "scipy.ndimage.label" if ndimage else "tests/components_np.py",
                                                            opt.host_calls),
             "launches per call: isa_cc_label %d, clean_instances %d (isa_cc_label %d + isa_cc_select LARGEST 5)"
             % (n_label, n_clean, n_label)]
    m = ReSeg(2, True, dtype=torch.float32)
    m.load_state_dict(R.synth_state_dict())
    m.eval()
    for kind in ("blobs", "noise"):
        maps_np = make_maps(kind, B, size, seed=size)
        maps = torch.from_numpy(maps_np).cuda()
        for conn in (4, 8):
            variants = {"label": lambda: m.cc_label(maps, conn),
                        "clean": lambda: m.clean_instances(maps, keep='largest', connectivity=conn)}
            got = [v.cpu().numpy() for v in variants["clean"]()]
            want = cnp.largest(maps_np, cnp.label(maps_np, conn)[0], 1, 255)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), "the device result differs from the restatement"
            host_out, host_count = host_clean(maps, conn)
            assert np.array_equal(host_out.cpu().numpy(), want[0]) and np.array_equal(host_count.cpu().numpy(), want[1])
            for fn in variants.values():                                  # warm-up: allocator, code objects
                fn()
            ms = {k: [] for k in variants}
            for _ in range(opt.calls):
                for k, fn in variants.items():
                    ms[k].append(timed_ms(fn))
            host = statistics.median(timed_ms(lambda: host_clean(maps, conn)) for _ in range(opt.host_calls))
            t_label, t_clean = statistics.median(ms["label"]), statistics.median(ms["clean"])
            comps = int(m.components(maps, connectivity=conn)[1].sum())
            lines.append("%-5s connectivity %d (%7d components)  label %7.3f ms  clean %7.3f ms  host %9.2f ms  host / clean %7.1f"
                         % (kind, conn, comps, t_label, t_clean, host, host / t_clean))
    x = R.synth_batch(B, size, size, seed=1)[0]
    seg = lambda: m.segment(x, max_objects=8)
    seg()
    t_seg = statistics.median(timed_ms(seg) for _ in range(5))
    lines.append("ReSeg.segment at 8 objects, [%d,21,%d,%d]: %.2f ms (median of 5 calls)" % (B, size, size, t_seg))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
