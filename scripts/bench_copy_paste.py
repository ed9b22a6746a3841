#!/usr/bin/env python3
"""Time of the loader's copy-paste stage on the device against the numpy restatement on the host.

A batch as RecordLoader holds it after torch.cat: rgb uint8 [B,size,size,3], sem uint8 [B,size,size], planes uint8
[B,size,size,32] (8 elliptical instances per image), already on the device; every image receives four instances of its
neighbour, flipped and shifted by up to half a side.  Timed, each as the median of --calls calls taken in turn after
--warmup, one event pair per call:
  entry    isa_copy_paste_u8 on buffers allocated once, outside the timed window: the launch that clears the counters and the
           three launches (areas, apply, compact);
  idle     the same entry with every source -1: every image passes through (the areas launch exits at once, apply copies,
           compact writes the plan) - the cost of the stage where nothing is pasted;
  stage    data.copy_paste as the loader calls it: sequences uploaded, outputs and scratch allocated;
  host     tests/copy_paste_np.py on the downloaded batch, the result uploaded; host clock around a device synchronise,
           median of --host-calls.
The entry's result is checked against the restatement on the whole batch.  Algorithmic bytes: every target pixel read
(c + 1 + k), every in-frame source pixel read (c + 1 + k), every pixel written (c + 1 + k).  No threshold: the script
reports.  Needs a GPU; there is no fallback.  Writes its lines to --out.  --trace-only runs the pasting entry alone, for
`rocprofv3 --kernel-trace` and scripts/prof_db.py (the duration of each launch)."""
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
import copy_paste_np as cpn  # noqa: E402  (the restatement the tests use: the self-check and the host side)
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
    ap.add_argument("--min-area", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--trace-only", action="store_true",
                    help="after the self-check, only --calls calls of the pasting entry: for a kernel trace of the launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "copy_paste_bench.txt"))
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_copy_paste.py needs the GPU"
    B, S, K, C = opt.batch, opt.size, 32, 3
    rgb_np, sem_np, planes_np = make_batch(B, S, seed=S)
    rng = np.random.default_rng(S + 1)
    counts = [8] * B
    xform = [((b + 1) % B, int(rng.integers(0, 4)), int(rng.integers(-S // 2, S // 2 + 1)), int(rng.integers(-S // 2, S // 2 + 1)))
             for b in range(B)]
    select = [0b01010101] * B
    rgb, sem, planes = (torch.from_numpy(a).cuda() for a in (rgb_np, sem_np, planes_np))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    nobj, xf, sel, idle_xf = i32(counts), i32(xform), i32(select), i32([(-1, 0, 0, 0)] * B)
    out = (torch.empty_like(rgb), torch.empty_like(sem), torch.empty_like(planes), torch.empty(B, dtype=torch.int32, device="cuda"),
           torch.empty((B, 4), dtype=torch.int32, device="cuda"))
    scratch = torch.empty((L.copy_paste_scratch_bytes(B, K),), dtype=torch.uint8, device="cuda")
    lib, st = L.lib(), L.stream_ptr()

    def entry_of(x):
        return lambda: L.check(lib.isa_copy_paste_u8(L.ptr(rgb), L.ptr(sem), L.ptr(planes), L.ptr(nobj), L.ptr(x), L.ptr(sel), B, S, S, C,
                                                     K, opt.min_area, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]),
                                                     L.ptr(out[4]), L.ptr(scratch), scratch.numel(), st), "isa_copy_paste_u8")

    def stage():
        return D.copy_paste(rgb, sem, planes, counts, [x[0] for x in xform], select, [x[1] for x in xform],
                            [x[2:] for x in xform], opt.min_area)

    def host():
        got = cpn.copy_paste(rgb.cpu().numpy(), sem.cpu().numpy(), planes.cpu().numpy(), counts, xform, select, opt.min_area)
        return [torch.from_numpy(a).cuda() for a in got[:4]]

    # self-check on the whole batch, bit for bit
    want = cpn.copy_paste(rgb_np, sem_np, planes_np, counts, xform, select, opt.min_area)
    entry_of(xf)()
    torch.cuda.synchronize()
    for name, g, w in zip(("rgb", "sem", "planes", "n_out"), out, want):
        assert np.array_equal(g.cpu().numpy(), w), "%s differs from the restatement" % name
    plan = want[4]
    in_frame = sum(max(0, S - abs(x[2])) * max(0, S - abs(x[3])) for x in xform)
    px = B * S * S
    algo = (2 * px + in_frame) * (C + 1 + K)

    if opt.trace_only:
        for _ in range(opt.calls):
            entry_of(xf)()
        torch.cuda.synchronize()
        return
    t_idle, t_entry, t_stage = alternate([entry_of(idle_xf), entry_of(xf), stage], opt.calls, opt.warmup)
    t_host = statistics.median(host_ms(host) for _ in range(opt.host_calls))
    lines = ["copy-paste bench: %s, batch [%d,%d,%d], %d planes, c = %d, min_area %d; median of %d alternating calls after %d "
             "warm-up, one event pair per call; host: the numpy restatement, copies included, median of %d calls"
             % (torch.cuda.get_device_name(0), B, S, S, K, C, opt.min_area, opt.calls, opt.warmup, opt.host_calls),
             "pasted planes per image %s, kept target planes %s, area-limited images %d, in-frame pixels %.0f %% of the batch"
             % (sorted(set(bin(int(p[0])).count("1") for p in plan)), sorted(set(bin(int(p[1])).count("1") for p in plan)),
                int(sum(p[3] for p in plan)), 100.0 * in_frame / px),
             "entry (clear + areas + apply + compact, preallocated) %7.1f us   algorithmic bytes %.1f MB = %.2f TB/s"
             % (t_entry * 1e3, algo / 1e6, algo / (t_entry * 1e-3) / 1e12),
             "entry, every image passing through              %7.1f us   algorithmic bytes %.1f MB = %.2f TB/s"
             % (t_idle * 1e3, 2 * px * (C + 1 + K) / 1e6, 2 * px * (C + 1 + K) / (t_idle * 1e-3) / 1e12),
             "stage (data.copy_paste: uploads and allocations)   %7.1f us" % (t_stage * 1e3),
             "host restatement %9.1f ms   host / stage %7.1f" % (t_host, t_host / t_stage)]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
