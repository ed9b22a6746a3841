#!/usr/bin/env python3
"""Time of tracing instance outlines: the device entry against a lower bound of any host tracer.

Maps uint8 [16,256,256] and [16,1024,1024], already on the device (where ReSeg.segment leaves them):
  "leaves":  32 elliptical instances on a background that covers most of the image (what a leaf map looks like);
  "uniform": the image cut into 32 rectangles, no background (long straight contours, few vertices);
  "checker": label against 0, pixel by pixel, traced under 4-connectivity: h w / 2 contours of four edges, the most
             contours a map can hold (the others are traced under 8-connectivity).
Timed:
  trace   isa_contour_trace alone (2 R + 9 launches, R = ceil(log4(4 h w))) into preallocated buffers with room for
          everything: device events around --reps back-to-back calls, the time of one call; the median of --calls windows.
  e2e     ReSeg.contours(labels, check=False) at those capacities: allocation of outputs and scratch + the entry; host
          clock around a device synchronise, median of --calls.
  host    labels.cpu(), then a vectorised numpy listing of the crack edges alone (four shifted comparisons and
          np.nonzero per image): no successor, no cycle, no vertex - a lower bound on any host tracer; median of
          --host-calls.
Needs a GPU; there is no fallback.  Writes its lines to --out."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import isa_amd  # noqa: F401,E402
import contours_np as C  # noqa: E402
from bench_props import event_ms, make_maps, timed_ms  # noqa: E402
from isa_amd import lib as L  # noqa: E402
from isa_amd.labelmaps import LabelOps  # noqa: E402


def maps_of(kind, B, size, seed):
    if kind == "checker":
        yy, xx = np.mgrid[0:size, 0:size]
        return np.broadcast_to(((yy + xx) % 2).astype(np.uint8), (B, size, size)).copy()
    return make_maps(kind, B, size, 32, seed)


def host_edges(labels):
    """The crack edges of every image as (y, x) index arrays per side: the first thing any host tracer computes."""
    lab = labels.cpu().numpy()
    out = []
    for img in lab:
        p = np.pad(img.astype(np.int16), 1, constant_values=-1)
        c = p[1:-1, 1:-1]
        fg = c != 0
        out.append([np.nonzero(fg & (c != nb)) for nb in (p[:-2, 1:-1], p[1:-1, 2:], p[2:, 1:-1], p[1:-1, :-2])])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contours_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_contours.py needs the GPU"
    B = opt.batch
    lib = L.checked()
    lines = ["contours bench: %s, maps uint8 [%d,S,S]; trace: device events around %d back-to-back isa_contour_trace calls, "
             "per call, median of %d windows; e2e: ReSeg.contours(check=False), host clock around a device synchronise, median "
             "of %d; host: labels.cpu() + numpy listing of the crack edges only, median of %d"
             % (torch.cuda.get_device_name(0), B, opt.reps, opt.calls, opt.calls, opt.host_calls)]
    m = LabelOps()
    for size in opt.sizes:
        for kind in ("leaves", "uniform", "checker"):
            conn = 4 if kind == "checker" else 8
            maps_np = maps_of(kind, B, size, seed=size)
            maps = torch.from_numpy(maps_np).cuda()
            _, _, found = m.contours(maps, connectivity=conn, check=False, max_contours=1, max_vertices=1)
            found = found.cpu().numpy()
            cmax, vmax = int(found[:, 0].max()), int(found[:, 1].max())
            table = torch.empty((B, cmax, 8), dtype=torch.int64, device="cuda")
            verts = torch.empty((B, vmax, 2), dtype=torch.int16, device="cuda")
            counts = torch.empty((B, 4), dtype=torch.int32, device="cuda")
            scratch = torch.empty((L.contour_scratch_bytes(B, size, size),), dtype=torch.uint8, device="cuda")
            st = L.stream_ptr()
            trace = lambda: lib.isa_contour_trace(maps, B, size, size, conn, cmax, vmax, table, verts, counts, scratch,
                                                  scratch.numel(), st)
            e2e = lambda: m.contours(maps, connectivity=conn, check=False, max_contours=cmax, max_vertices=vmax)
            trace()
            if size <= 256:                                                  # the restatement is sequential Python
                wt, wv, wc = C.trace(maps_np[:1], conn, cmax, vmax)
                k, v = int(wc[0, 0]), int(wc[0, 1])
                assert np.array_equal(counts[:1].cpu().numpy(), wc) and np.array_equal(table[0, :k].cpu().numpy(), wt[0, :k]) \
                    and np.array_equal(verts[0, :v].cpu().numpy(), wv[0, :v]), "the device result differs from the restatement"
            assert int(counts[:, 2:].sum()) == 0
            edges = int(table[0, :int(counts[0, 0]), 3].sum())
            for fn in (trace, e2e):                                          # warm-up: allocator, code objects
                fn()
            ms = {"trace": [], "e2e": []}
            for _ in range(opt.calls):
                ms["trace"].append(event_ms(trace, opt.reps))
                ms["e2e"].append(timed_ms(e2e))
            host = statistics.median(timed_ms(lambda: host_edges(maps)) for _ in range(opt.host_calls))
            t = {name: statistics.median(v) for name, v in ms.items()}
            lines.append("S %4d  %-7s conn %d  image 0: %7d contours %8d vertices %8d edges  scratch %7.1f MiB  trace %8.3f ms  "
                         "e2e %8.3f ms  host edges only %9.2f ms  host / e2e %7.1f"
                         % (size, kind, conn, int(counts[0, 0]), int(counts[0, 1]), edges, scratch.numel() / 2 ** 20, t["trace"],
                            t["e2e"], host, host / t["e2e"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
