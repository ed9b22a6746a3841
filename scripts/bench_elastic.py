#!/usr/bin/env python3
"""Time of the loader's elastic stage on the device against the host way.

A batch as RecordLoader holds it after torch.cat: rgb uint8 [B,size,size,3], sem uint8 [B,size,size], planes uint8
[B,size,size,32] (8 elliptical instances per image), already on the device.  Timed, each as the median of --calls calls
taken in turn after --warmup, one event pair per call.  The first five call the entry points themselves on buffers
allocated once, outside the timed window; the sixth is the stage as the loader runs it, allocations and the download of
the plane sums included:
  field    isa_elastic_field (2 launches), noise [B,size,size,2] -> disp;
  rgb      isa_warp_u8, c = 3, bilinear;
  sem      isa_warp_u8, c = 1, nearest;
  planes   isa_warp_u8, c = 32, nearest;
  sums     isa_plane_sums_u8 over the warped planes (the compaction's test; no plane is emptied at these settings);
  stage    data.elastic_field + data.elastic: the five above behind the host functions;
  host     the same work the host way: the batch downloaded, scipy.ndimage.gaussian_filter of the noise (mode='constant'),
           map_coordinates per channel (order 1 for the image, order 0 for the annotation, mode='nearest': 36 calls per
           image), the result uploaded; host clock around a device synchronise, median of --host-calls.
The device results are checked against the restatement the tests use on the first two images.  No threshold: the script
reports.  Needs a GPU; there is no fallback.  Writes its lines to --out."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import isa_amd  # noqa: F401,E402
import elastic_np as en  # noqa: E402  (the restatement the tests use: the self-check below)
from isa_amd import data as D  # noqa: E402
from isa_amd import lib as L  # noqa: E402


def make_batch(B, size, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    planes = np.zeros((B, size, size, 32), np.uint8)
    for b in range(B):
        for k in range(8):
            cy, cx = rng.uniform(0.15, 0.85, 2) * size
            ry, rx = rng.uniform(0.05, 0.14, 2) * size
            planes[b, :, :, k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    rgb = rng.integers(0, 256, (B, size, size, 3), dtype=np.uint8)
    return rgb, (planes.sum(3) > 0).astype(np.uint8), planes


def host_stage(rgb, sem, planes, noise, alpha, sigma):
    """The stage the host way: download, scipy, upload."""
    from scipy.ndimage import gaussian_filter, map_coordinates
    r, s, p, z = rgb.cpu().numpy(), sem.cpu().numpy(), planes.cpu().numpy(), noise.cpu().numpy()
    B, h, w = s.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r2, s2, p2 = np.empty_like(r), np.empty_like(s), np.empty_like(p)
    for b in range(B):
        dx = alpha[b] * gaussian_filter(z[b, :, :, 0], sigma, mode='constant', cval=0.0)
        dy = alpha[b] * gaussian_filter(z[b, :, :, 1], sigma, mode='constant', cval=0.0)
        coords = np.stack([yy + dy, xx + dx])
        for k in range(3):
            r2[b, :, :, k] = map_coordinates(r[b, :, :, k], coords, order=1, mode='nearest')
        s2[b] = map_coordinates(s[b], coords, order=0, mode='nearest')
        for k in range(p.shape[3]):
            p2[b, :, :, k] = map_coordinates(p[b, :, :, k], coords, order=0, mode='nearest')
    return torch.from_numpy(r2).cuda(), torch.from_numpy(s2).cuda(), torch.from_numpy(p2).cuda()


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
    ap.add_argument("--sigma", type=float, default=8.0)
    ap.add_argument("--alpha", type=float, default=100.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elastic_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_elastic.py needs the GPU"
    B, S = opt.batch, opt.size
    rgb_np, sem_np, planes_np = make_batch(B, S, seed=S)
    rgb, sem, planes = (torch.from_numpy(a).cuda() for a in (rgb_np, sem_np, planes_np))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(S)
    noise = torch.rand((B, S, S, 2), generator=gen, device="cuda") * 2 - 1
    alpha = [opt.alpha] * B
    taps, radius = D.gaussian_taps(opt.sigma)

    # self-check on the first two images: the field within the tests' bound, the warps bit for bit
    disp = D.elastic_field(noise, alpha, opt.sigma)
    want = en.field(noise[:2].cpu().numpy(), alpha[:2], taps)
    assert np.abs(disp[:2].cpu().numpy() - want).max() <= opt.alpha * (4 * radius + 8) * 2.0 ** -24, "the field differs"
    r2, s2, p2, counts = D.elastic(rgb, sem, planes, [8] * B, disp)
    d2 = disp[:2].cpu().numpy()
    assert np.array_equal(r2[:2].cpu().numpy(), en.warp_bilinear(rgb_np[:2], d2)), "the image warp differs"
    assert np.array_equal(s2[:2].cpu().numpy(), en.warp_nearest(sem_np[:2], d2)), "the semantic warp differs"
    assert np.array_equal(p2[:2].cpu().numpy(), en.warp_nearest(planes_np[:2], d2)), "the plane warp differs"

    lib, st = L.lib(), L.stream_ptr()
    a_dev = torch.tensor(alpha, dtype=torch.float32, device="cuda")
    scratch = torch.empty((L.elastic_scratch_bytes(B, S, S),), dtype=torch.uint8, device="cuda")
    out_d, out_r, out_s, out_p = torch.empty_like(disp), torch.empty_like(rgb), torch.empty_like(sem), torch.empty_like(planes)
    sums = torch.zeros((B, 32), dtype=torch.int64, device="cuda")
    tp = taps.ctypes.data_as(C.c_void_p)

    def field():
        L.check(lib.isa_elastic_field(L.ptr(noise), L.ptr(a_dev), B, S, S, tp, radius, L.ptr(out_d), L.ptr(scratch),
                                      scratch.numel(), st), "isa_elastic_field")

    def warp_of(src, c, mode, dst):
        return lambda: L.check(lib.isa_warp_u8(L.ptr(src), L.ptr(disp), B, S, S, c, mode, L.ptr(dst), st), "isa_warp_u8")

    def plane_sums():
        L.check(lib.isa_plane_sums_u8(L.ptr(out_p), B, S, S, 32, 0, 0, S, S, L.ptr(sums), st), "isa_plane_sums_u8")

    def stage():
        return D.elastic(rgb, sem, planes, [8] * B, D.elastic_field(noise, alpha, opt.sigma))

    variants = [field, warp_of(rgb, 3, L.WARP_BILINEAR, out_r), warp_of(sem, 1, L.WARP_NEAREST, out_s),
                warp_of(planes, 32, L.WARP_NEAREST, out_p), plane_sums, stage]
    t_field, t_rgb, t_sem, t_planes, t_sums, t_stage = alternate(variants, opt.calls, opt.warmup)
    assert torch.equal(out_d, disp) and torch.equal(out_r, r2) and torch.equal(out_s, s2)
    assert counts != [8] * B or torch.equal(out_p, p2)
    t_host = statistics.median(host_ms(lambda: host_stage(rgb, sem, planes, noise, alpha, opt.sigma)) for _ in range(opt.host_calls))
    mb = lambda t: t.numel() * t.element_size() / 1e6
    lines = ["elastic bench: %s, batch [%d,%d,%d], sigma %g (radius %d), alpha %g; median of %d alternating calls after %d "
             "warm-up, one event pair per call; host: scipy.ndimage gaussian_filter + map_coordinates per channel, copies "
             "included, median of %d calls" % (torch.cuda.get_device_name(0), B, S, S, opt.sigma, radius, opt.alpha, opt.calls,
                                               opt.warmup, opt.host_calls),
             "entries on preallocated buffers: field (2 launches, %.1f MB noise, %.1f MB scratch written and read, %.1f MB "
             "field) %7.3f ms" % (mb(noise), mb(noise), mb(disp), t_field),
             "  warp rgb c=3 bilinear %7.3f ms   warp sem c=1 nearest %7.3f ms   warp planes c=32 nearest (%.1f MB in, %.1f MB "
             "out, %.1f MB field) %7.3f ms = %.2f TB/s   plane sums %7.3f ms"
             % (t_rgb, t_sem, mb(planes), mb(planes), mb(disp), t_planes, (2 * mb(planes) + mb(disp)) / t_planes / 1e3, t_sums),
             "  sum of the six launches %7.3f ms" % (t_field + t_rgb + t_sem + t_planes + t_sums),
             "stage (data.elastic_field + data.elastic: the same launches, allocations, the sums read back; planes kept %s) "
             "%7.3f ms" % (sorted(set(counts)), t_stage),
             "host stage %9.1f ms   host / stage %7.1f" % (t_host, t_host / t_stage)]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
