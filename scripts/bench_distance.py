#!/usr/bin/env python3
"""Time of the distance transform to the two nearest instances and of what is built on it, against the host way.

Label maps uint8 [B,size,size] already on the device (where the step's targets and ReSeg.segment's output live):
  "blobs8" : 8 elliptical instances per image (a training target);
  "holes"  : the same with every instance eroded to its core and speckles of background in it (a cleaned prediction:
             unexplained foreground all around the instances);
  "single" : one instance per image (no second instance: the walk of the row pass is bounded by d1 alone);
  "pair"   : two single pixels in opposite corners (the longest walk the pruning allows at this size).
Timed, each as the median of --calls calls taken in turn after --warmup, one event pair per call.  The first three call
the entry points themselves on buffers allocated once, outside the timed window (what the training step does: its
buffers come from the step's arena); the fourth is the Python method, allocations included:
  edt      isa_edt2_u8 alone, all three outputs (2 launches);
  weights  isa_edt2_u8 (d1sq, d2sq) + isa_border_weights (3 launches);
  fill     isa_edt2_u8 (d1sq, nearest) + isa_fill_labels (4 launches);
  method   ReSeg.fill_instances: the same four launches behind the method, which allocates its outputs and the scratch;
  host     the fill the host way: labels.cpu(), one scipy.ndimage.distance_transform_edt per instance, arg-min, the fill
           and the copy back; host clock around a device synchronise, median of --host-calls.
Then a whole training step (B, size, bf16, instance head on, hipGraph replay) with the border term on and off, the two
called alternately, same protocol.  No threshold: the script reports.  Needs a GPU; there is no fallback.  Writes its
lines to --out."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import isa_amd  # noqa: F401,E402
import distance_np as dn  # noqa: E402  (the restatement the tests use: the self-check below, as bench_components.py does)
from isa_amd import lib as L  # noqa: E402
from isa_amd.labelmaps import LabelOps  # noqa: E402
from isa_amd.reseg import ReSeg  # noqa: E402
from isa_amd.trainer import Trainer  # noqa: E402


def make_maps(kind, B, size, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((B, size, size), np.uint8)
    if kind == "pair":
        m[:, 0, 0], m[:, size - 1, size - 1] = 1, 2
        return m, np.ones_like(m)
    yy, xx = np.mgrid[0:size, 0:size]
    fg = np.zeros_like(m)
    for b in range(B):
        for k in range(1 if kind == "single" else 8):
            cy, cx = rng.uniform(0.15, 0.85, 2) * size
            ry, rx = rng.uniform(0.05, 0.14, 2) * size
            r2 = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
            free = m[b] == 0
            fg[b][(r2 <= 1.0) & free] = 1
            m[b][(r2 <= (0.5 if kind == "holes" else 1.0)) & free & ((fg[b] == 1) | (kind != "holes"))] = k + 1
    if kind == "holes":
        m[(rng.random(m.shape) < 0.05)] = 0
    return m, (fg if kind == "holes" else np.ones_like(m))


def host_fill(labels, fg):
    """fill_instances the host way: the copy down, one scipy EDT per instance, the nearest label, the copy back."""
    from scipy.ndimage import distance_transform_edt
    lab, f = labels.cpu().numpy(), fg.cpu().numpy()
    out = lab.copy()
    for b, img in enumerate(lab):
        ks = [int(k) for k in np.unique(img) if k]
        if not ks:
            continue
        D = np.stack([distance_transform_edt(img != k) for k in ks])
        near = np.asarray(ks, np.uint8)[np.argmin(D, axis=0)]
        take = (img == 0) & (f[b] != 0)
        out[b][take] = near[take]
    return torch.from_numpy(out).cuda()


def timed_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, calls, warmup):
    """Median ms of each function, called in turn."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(calls):
        for i, f in enumerate(fns):
            ts[i].append(timed_ms(f))
    return [statistics.median(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_distance.py needs the GPU"
    B, S = opt.batch, opt.size
    lines = ["distance bench: %s, maps uint8 [%d,%d,%d]; median of %d alternating calls after %d warm-up, one event pair per "
             "call; host: scipy.ndimage.distance_transform_edt per instance, copies included, median of %d calls"
             % (torch.cuda.get_device_name(0), B, S, S, opt.calls, opt.warmup, opt.host_calls),
             "edt / weights / fill: the entry points on preallocated buffers (2 / 3 / 4 launches); method: ReSeg.fill_instances, "
             "allocations included"]
    m = LabelOps()
    for kind in ("blobs8", "holes", "single", "pair"):
        maps_np, fg_np = make_maps(kind, B, S, seed=S)
        maps, fg = torch.from_numpy(maps_np).cuda(), torch.from_numpy(fg_np).cuda()
        got = [t.cpu().numpy() for t in m.distance_transform(maps)]
        want = dn.edt2(maps_np[:2])
        assert all(np.array_equal(g[:2], w) for g, w in zip(got, want)), "the device result differs from the restatement"
        filled, count = m.fill_instances(maps, fg)
        # scipy's float distances order ties like the integers only by luck: compare where the nearest label is unique
        host = host_fill(maps, fg).cpu().numpy()
        unique = got[0] != got[1]
        assert np.array_equal(host[unique], filled.cpu().numpy()[unique]), "the host fill differs from the device fill"
        lib, st = L.lib(), L.stream_ptr()
        i32 = lambda: torch.empty((B, S, S), dtype=torch.int32, device="cuda")
        d1, d2, near, out = i32(), i32(), torch.empty_like(maps), torch.empty_like(maps)
        wmap, nfill = torch.empty((B, S, S), device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")
        scratch = torch.empty((L.edt_scratch_bytes(B, S, S),), dtype=torch.uint8, device="cuda")
        cfg = torch.tensor([10.0, 5.0], device="cuda")

        def edt(a, b, c):
            L.check(lib.isa_edt2_u8(L.ptr(maps), B, S, S, L.ptr(a), L.ptr(b), L.ptr(c), L.ptr(scratch), scratch.numel(), st),
                    "isa_edt2_u8")

        def weights():
            edt(d1, d2, None)
            L.check(lib.isa_border_weights(L.ptr(maps), L.ptr(d1), L.ptr(d2), L.ptr(cfg), B, S * S, L.ptr(wmap), st),
                    "isa_border_weights")

        def fill():
            edt(d1, None, near)
            L.check(lib.isa_fill_labels(L.ptr(maps), L.ptr(fg), L.ptr(near), L.ptr(d1), -1, B, S * S, L.ptr(out), L.ptr(nfill),
                                        st), "isa_fill_labels")

        variants = [lambda: edt(d1, d2, near), weights, fill, lambda: m.fill_instances(maps, fg)]
        t_edt, t_w, t_fill, t_method = alternate(variants, opt.calls, opt.warmup)
        assert torch.equal(out, filled) and torch.equal(nfill, count)
        t_host = statistics.median(host_ms(lambda: host_fill(maps, fg)) for _ in range(opt.host_calls))
        lines.append("%-7s (%7d labelled, %7d filled)  edt %7.3f ms  weights %7.3f ms  fill %7.3f ms  method %7.3f ms  "
                     "host fill %9.2f ms  host / method %7.1f" % (kind, int((maps_np != 0).sum()), int(count.sum()), t_edt, t_w,
                                                                  t_fill, t_method, t_host, t_host / t_method))
    del m
    torch.cuda.empty_cache()
    if not opt.no_step:
        from isa_amd.data import synth_batch
        x, sem_t, ins, n = synth_batch(B, S, S, seed=100)
        x, sem_t, ins = x.cuda(), sem_t.cuda(), ins.cuda()
        sel = [list(range(int(k))) for k in n.view(-1)]
        steps = []
        for w in (0.0, 10.0):
            net = ReSeg(2, True, dtype=torch.bfloat16)
            net.reset_parameters(seed=23)
            net.train()
            tr = Trainer(net, border_weight=w, border_sigma=5.0)
            steps.append(lambda tr=tr: tr.train_step_graphed(x, sem_t, ins, n, selected_idx=sel))
        t_0, t_1 = alternate(steps, opt.calls, opt.warmup)
        lines.append("train step (bf16, instance head on, hipGraph replay): border term off %8.3f ms   on %8.3f ms   "
                     "difference %+.3f ms (on: the K-class criterion kernels in place of the 2-class ones, the label map, the "
                     "transform and the weight map)" % (t_0, t_1, t_1 - t_0))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
