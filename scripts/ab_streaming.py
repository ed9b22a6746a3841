#!/usr/bin/env python3
"""A/B of the streaming walkers (isa_bn_bwd_reduce / _apply, isa_affine_act_res, isa_axpy) between two builds of the
kernel library: are the outputs bit-identical, and what is the device time of each.

    python scripts/ab_streaming.py --base PATH/libisa_kernels.so [--new PATH/libisa_kernels.so] [--out DIR]

--base is a build of the commit to compare against (a scratch checkout built with `make -C .../csrc`), --new defaults to
the library in the tree.  Each build runs in a process of its own (ISA_KERNELS_LIB selects it), under its own time
limit; the second starts only if the first ended well.  This process never touches the GPU.

Shapes: the launches of a 256x256, batch 16, bf16 training step that profiles/r03_step_shapes.txt lists for these entry
points (bytes = tensors touched x tensor size).  Inputs are seeded, so both builds see the same bits.  Per row:
  * identical: the output tensor of apply / materialise / axpy must be bit-identical between the builds; the reduce rows
    (float atomics, unordered in both builds) must agree within SUM_BOUND = 1e-5 of their sums of |terms|;
  * time: operands rotate over enough independent sets that no launch finds its inputs in the 256 MB Infinity Cache
    (as KBENCH_ROTATE in scripts/kbench.py); REPEATS event-timed loops per row give the median and the spread
    (max - min) of each build.  A row is slower when new median - base median exceeds the base build's own spread.
Exit status 1 when an output differs or a row is slower.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM_BOUND = 1e-5
REPEATS = 5
B = 16
# entry point, h = w, channels, MB per launch as r03_step_shapes.txt counts them
ROWS = [("reduce", 256, 64, 268), ("reduce", 128, 128, 134), ("reduce", 64, 256, 67), ("reduce", 32, 512, 33.5),
        ("reduce", 16, 1024, 16.8), ("apply", 256, 64, 402), ("apply", 64, 256, 100), ("apply", 32, 512, 50),
        ("apply", 16, 1024, 25), ("materialise", 256, 64, 402), ("materialise", 256, 32, 201), ("axpy", 128, 64, 100),
        # the variants with per-image multipliers (Dropout2d masks): apply with bscale, materialise with bscale and oscale
        ("apply+bscale", 64, 256, 100), ("materialise+scales", 128, 64, 100)]


def worker(out_path):
    sys.path[:0] = [ROOT]
    import torch
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    lib = L.lib()
    st = L.stream_ptr()
    dtype = torch.bfloat16
    res = {"lib": L.LIB_PATH, "rows": []}
    for kind, hw, c, mb in ROWS:
        ntens = 2 if kind in ("reduce", "axpy") else 3
        tbytes = B * hw * hw * c * 2
        nsets = max(2, min(24, -(-(640 << 20) // (ntens * tbytes))))
        gen = torch.Generator(device="cuda").manual_seed(1000 + hw + c)

        def tens(scale=1.0, offset=0.0):
            return (torch.randn(B, hw, hw, c, device="cuda", generator=gen) * scale + offset).to(dtype)

        def desc(t):
            return L.IsaTensor(t.data_ptr(), B, hw, hw, c, c, L.dtype_code(dtype), 1)
        sc = (torch.rand(c, device="cuda", generator=gen) + 0.5).contiguous()
        sh = torch.randn(c, device="cuda", generator=gen).contiguous()
        mean = (torch.randn(c, device="cuda", generator=gen) * 0.5).contiguous()
        inv = (torch.rand(c, device="cuda", generator=gen) + 0.5).contiguous()
        redin = torch.randn(8 * 2 * c, device="cuda", generator=gen).contiguous()
        gamma = torch.ones(c, device="cuda")
        mask = ((torch.rand(B, c, device="cuda", generator=gen) > 0.2).float() * 1.25).contiguous()
        mask2 = ((torch.rand(B, c, device="cuda", generator=gen) > 0.2).float() * 1.25).contiguous()
        pi = "+" in kind
        pro = L.IsaPro(L.addr(sc), L.addr(sh), L.addr(mask) if pi else None, L.ACT_RELU6, None)
        count = float(B * hw * hw)
        sets = []
        for _ in range(nsets):
            a, b_, o = tens(), tens(2.0, 0.5), tens()
            red = torch.zeros(8 * 2 * c, device="cuda")
            da, db, do = desc(a), desc(b_), desc(o)
            if kind == "reduce":
                fn = (lambda da=da, db=db, red=red: lib.isa_bn_bwd_reduce(
                    C.byref(da), C.byref(db), L.ptr(sc), L.ptr(sh), L.ptr(mean), L.ptr(inv), L.ACT_RELU6, None, L.ptr(red), st))
            elif kind.startswith("apply"):
                fn = (lambda da=da, db=db, do=do: lib.isa_bn_bwd_apply(
                    C.byref(da), C.byref(db), L.ptr(sc), L.ptr(sh), L.ptr(mean), L.ptr(inv), L.ACT_RELU6,
                    L.ptr(mask) if pi else None, L.ptr(gamma),
                    L.ptr(redin), count, 1, C.byref(do), None, None, st))
            elif kind.startswith("materialise"):
                fn = (lambda da=da, db=db, do=do: lib.isa_affine_act_res(C.byref(db), C.byref(pro), C.byref(da), None,
                                                                         L.ptr(mask2) if pi else None, C.byref(do), st))
            else:
                fn = (lambda da=da, do=do: lib.isa_axpy(C.byref(da), C.byref(do), -1.5, 1, st))
            sets.append((fn, a, b_, o, red, (da, db, do)))
        # outputs of one launch on set 0, from the seeded inputs
        fn, a, b_, o, red, _ = sets[0]
        L.check(fn(), kind)
        torch.cuda.synchronize()
        row = {"kind": kind, "hw": hw, "c": c, "mb": mb, "nsets": nsets}
        if kind == "reduce":
            z = b_.double() * sc.double() + sh.double()
            dz = a.double() * ((z.float() > 0) & (z.float() < 6)).double()
            yh = (b_.double() - mean.double()) * inv.double()
            row["sums"] = red.view(8, 2 * c).double().sum(0).cpu().tolist()
            row["mag"] = torch.cat([dz.abs().sum((0, 1, 2)), (dz * yh).abs().sum((0, 1, 2))]).cpu().tolist()
            del z, dz, yh
        else:
            row["sha256"] = hashlib.sha256(o.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
        # timing: every launch on the next operand set
        for f in sets:
            f[0]()
        torch.cuda.synchronize()
        loops = max(2, 96 // nsets)
        times = []
        for _ in range(REPEATS):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(loops):
                for f in sets:
                    f[0]()
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e) * 1e3 / (loops * nsets))
        row["us"] = times
        res["rows"].append(row)
        print("%-18s %4d x %-5d %s" % (kind, hw, c, " ".join("%.1f" % t for t in times)), flush=True)
        del sets
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(res, f)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def compare(base, new):
    bad = False
    print("%-18s %-11s %6s | %9s %7s | %9s %7s | %6s %7s  %s" % ("entry point", "shape", "MB", "base us", "spread", "new us",
                                                                 "spread", "ratio", "GB/s", "outputs"))
    for rb, rn in zip(base["rows"], new["rows"]):
        assert (rb["kind"], rb["hw"], rb["c"]) == (rn["kind"], rn["hw"], rn["c"])
        if rb["kind"] == "reduce":
            err = max(abs(x - y) / max(m, 1e-30) for x, y, m in zip(rb["sums"], rn["sums"], rb["mag"]))
            same = err < SUM_BOUND
            what = "sums within %.1e (bound %.0e)" % (err, SUM_BOUND)
        else:
            same = rb["sha256"] == rn["sha256"]
            what = "bit-identical" if same else "DIFFERENT"
        mb_, mn = median(rb["us"]), median(rn["us"])
        sb, sn = max(rb["us"]) - min(rb["us"]), max(rn["us"]) - min(rn["us"])
        slower = mn - mb_ > sb
        bad = bad or slower or not same
        print("%-18s %4dx%-3dx%-4d %6.1f | %9.1f %7.1f | %9.1f %7.1f | %6.2f %7.0f  %s%s" % (
            rb["kind"], rb["hw"], rb["hw"], rb["c"], rb["mb"], mb_, sb, mn, sn, mb_ / mn, rb["mb"] * 1e3 / mn, what,
            "  SLOWER" if slower else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base")
    ap.add_argument("--new", default=os.path.join(ROOT, "instance-segmentation-attention_amd", "libisa_kernels.so"))
    ap.add_argument("--out", default="ab_streaming_out")
    ap.add_argument("--limit", type=int, default=300, help="seconds per build")
    ap.add_argument("--kinds", default="", help="comma-separated subset of the entry-point names in ROWS")
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.kinds:
        ROWS[:] = [r for r in ROWS if r[0] in a.kinds.split(",")]
    if a.worker:
        return worker(a.worker)
    if not a.base:
        ap.error("--base is required")
    os.makedirs(a.out, exist_ok=True)
    files = []
    for tag, path in (("base", a.base), ("new", a.new)):
        out = os.path.join(a.out, "ab_streaming_%s.json" % tag)
        env = dict(os.environ, ISA_KERNELS_LIB=os.path.abspath(path))
        print("== %s: %s" % (tag, path), flush=True)
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", out, "--kinds", a.kinds],
                             env=env)
        if rc != 0:                      # a fault, an abort or the time limit: nothing more starts on the GPU
            print("%s build ended with status %d" % (tag, rc))
            return rc
        files.append(out)
    return compare(*[json.load(open(f)) for f in files])


if __name__ == "__main__":
    sys.exit(main())
