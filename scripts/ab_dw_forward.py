#!/usr/bin/env python3
"""A/B of the depthwise kernels (isa_dwconv3x3, isa_dwconv3x3_dgrad, isa_dwconv3x3_bn_backward, bf16) between two builds
of the kernel library: are the outputs bit-identical, and what is the device time of a launch on HBM-cold operands.

    python scripts/ab_dw_forward.py --base PATH/libisa_kernels.so [--new PATH/libisa_kernels.so] [--out DIR]
    python scripts/ab_dw_forward.py --compare [--out DIR]          (the table again, from the two result files)

--base is a build of the commit to compare against, --new defaults to the library in the tree.  Each build runs in a
process of its own (ISA_KERNELS_LIB selects it), under its own time limit; the second starts only if the first ended
well.  This process never touches the GPU.  (Modelled on scripts/ab_fixed_cost.py.)

Rows: the depthwise shapes of a 256x256, batch 16, bf16 training step (profiles/fixed_cost_step_shapes.txt: the 537 /
134 / 67 / 34 MB launches of isa_dwconv3x3, the 1074 / 537 / 268 / 134 / 67 / 34 MB launches of
isa_dwconv3x3_bn_backward) and tiny ones, where a launch is nothing but its prologue and its fold.  Inputs are seeded,
so both builds see the same bits.  Per row:
  * y / dx and the weight-gradient slabs (one per workgroup, no atomics) must be bit-identical between the builds;
  * the statistics rows of the forward and the BN(x) sums of the backward (float atomics into 8 replicas, unordered in
    both builds) must agree within SUM_BOUND = 1e-5 of their sums of |terms|;
  * time: the operand sets rotate so that no launch finds its inputs in the 256 MB Infinity Cache (KBENCH_ROTATE in
    scripts/kbench.py); REPEATS event-timed loops give the median and the spread (max - min) of each build.  The time
    is that of the entry point (the backward: kernel plus second-stage reduce).
Exit status 1 when an output differs, or when a row's new median exceeds the base median by more than the base spread.
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
CB = 32
# kind, images, h = w, channels, variant.  fwd: prologue form ("relu6": scale / shift + ReLU6 and statistics, as every
# depthwise conv of the step; "none": no prologue, bias, no statistics); dgrad: accumulate; bwd: xmode (1: ReLU6 prologue
# + BN(x) sums, 0: plain x)
ROWS = [("fwd", 16, 256, 128, "relu6"), ("fwd", 16, 128, 128, "relu6"), ("fwd", 16, 256, 32, "relu6"), ("fwd", 16, 64, 256, "relu6"),
        ("fwd", 16, 64, 128, "relu6"), ("fwd", 16, 32, 512, "relu6"), ("fwd", 16, 256, 128, "none"),
        ("fwd", 16, 8, 64, "relu6"), ("fwd", 2, 5, 24, "relu6"), ("fwd", 1, 1, 64, "none"),
        ("dgrad", 16, 256, 128, 0), ("dgrad", 16, 128, 128, 1), ("dgrad", 16, 8, 64, 0),
        ("bwd", 16, 256, 128, 1), ("bwd", 16, 256, 64, 1), ("bwd", 16, 128, 128, 1), ("bwd", 16, 64, 256, 1),
        ("bwd", 16, 64, 128, 1), ("bwd", 16, 32, 256, 1), ("bwd", 16, 128, 128, 0),
        ("bwd", 16, 8, 64, 1), ("bwd", 2, 5, 24, 0), ("bwd", 1, 1, 64, 1)]


def worker(out_path):
    sys.path[:0] = [ROOT]
    import torch
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    from isa_amd.engine import Engine, ParamStore
    lib = L.lib()
    st = L.stream_ptr()
    bf = torch.bfloat16
    ws = torch.zeros(16 << 20, device="cuda")
    res = {"lib": L.LIB_PATH, "rows": []}
    for kind, B, hw, c, var in ROWS:
        M = B * hw * hw
        gen = torch.Generator(device="cuda").manual_seed(11 + c + 3 * hw + B)
        ntens = 4 if kind == "bwd" else 2
        nsets = max(2, min(24, -(-(640 << 20) // (ntens * M * c * 2))))
        ps = ParamStore([("wd", (c, 1, 3, 3)), ("b", (c,))], "cuda")
        ps.load_state_dict({"wd": torch.randn(c, 1, 3, 3, generator=torch.Generator().manual_seed(5)) / 3,
                            "b": torch.randn(c, generator=torch.Generator().manual_seed(6))})
        eng = Engine(ps, bf)
        eng.begin(True, False)
        reg = eng.reg_dw("wd")
        eng.packer.pack()

        def tens(scale=1.0, offset=0.0):
            return (torch.randn(B, hw, hw, c, device="cuda", generator=gen) * scale + offset).to(bf)

        def desc(t):
            return L.IsaTensor(t.data_ptr(), B, hw, hw, c, c, L.dtype_code(bf), 1)

        def vec(lo=0.5):
            return (torch.rand(c, device="cuda", generator=gen) + lo).contiguous()
        keep, sets = [], []
        sc, sh = vec(), vec(-0.5)
        if kind == "fwd":
            pro = L.IsaPro(L.addr(sc), L.addr(sh), None, L.ACT_RELU6, None) if var == "relu6" else None
            for _ in range(nsets):
                x, y = tens(2.0), tens()
                stats = torch.zeros(8 * 2 * c, device="cuda") if var == "relu6" else None
                d = [desc(x), desc(y)]
                keep.append((d, x, y, stats))
                fn = (lambda d=d, stats=stats: lib.isa_dwconv3x3(
                    C.byref(d[0]), C.byref(pro) if pro else None, eng.packer.ptr(reg["fwd"]),
                    None if var == "relu6" else ps.ptr("b"), C.byref(d[1]), L.ptr(stats), st))
                sets.append((fn, y, stats, None))
        elif kind == "dgrad":
            for _ in range(nsets):
                dy, dx = tens(), tens()
                d = [desc(dy), desc(dx)]
                keep.append((d, dy, dx))
                fn = (lambda d=d: lib.isa_dwconv3x3_dgrad(C.byref(d[0]), eng.packer.ptr(reg["dgrad"]), C.byref(d[1]), int(var), st))
                sets.append((fn, dx, None, None))
        else:
            ymu, yis, xmu, xis = vec(), vec(), vec(0.0), vec()
            yred = torch.zeros(8 * 2 * c, device="cuda")
            yred[:2 * c] = torch.randn(2 * c, device="cuda", generator=gen) * M * 0.01
            dgam, dbet = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
            dw = torch.zeros(c, 1, 3, 3, device="cuda")
            for _ in range(nsets):
                g, y, x, dx = tens(), tens(2.0, 1.0), tens(2.0), tens()
                xred = torch.zeros(8 * 2 * c, device="cuda")
                ybn = L.IsaBnBwd(L.addr(sc), L.addr(sh), L.addr(ymu), L.addr(yis), L.addr(yred), None, L.addr(dgam),
                                 L.addr(dbet), float(M), L.ACT_RELU6)
                xbn = L.IsaBnBwd(L.addr(sc), L.addr(sh), L.addr(xmu), L.addr(xis), None, L.addr(xred), None, None, 1.0, 0)
                xpro = L.IsaPro(L.addr(sc), L.addr(sh), None, L.ACT_RELU6, None)
                d = [desc(g), desc(y), desc(x), desc(dx)]
                keep.append((ybn, xbn, xpro, d, g, y, x))
                fn = (lambda d=d, ybn=ybn, xbn=xbn, xpro=xpro: lib.isa_dwconv3x3_bn_backward(
                    C.byref(d[0]), C.byref(d[1]), C.byref(ybn), C.byref(d[2]), C.byref(xpro) if var else None,
                    C.byref(xbn) if var else None, eng.packer.ptr(reg["dgrad"]), L.ptr(dw), c, C.byref(d[3]), 0, None,
                    L.ptr(ws), ws.numel(), None, st))
                sets.append((fn, dx, xred if var else None, x))
        # outputs of one launch on set 0, from the seeded inputs
        fn, out, sums, x = sets[0]
        L.check(fn(), kind)
        torch.cuda.synchronize()

        def sha(t):
            return hashlib.sha256(t.contiguous().view(torch.int16 if t.dtype == bf else torch.int32).cpu().numpy().tobytes()).hexdigest()
        row = {"kind": kind, "B": B, "hw": hw, "c": c, "var": var, "nsets": nsets, "mb": ntens * M * c * 2 / 1e6, "out": sha(out)}
        if kind == "bwd":
            ncb = -(-c // CB)
            tiles = B * -(-hw // 8) * -(-hw // 32)
            gx = max(1, min(256 // ncb, tiles, ws.numel() // (10 * CB * ncb)))
            row["slabs"] = sha(ws[:gx * ncb * 10 * CB])
        if sums is not None:
            row["sums"] = sums.view(8, 2 * c).double().sum(0).cpu().tolist()
            o = out.double()
            if kind == "fwd":
                row["mag"] = torch.cat([o.abs().sum((0, 1, 2)), (o * o).sum((0, 1, 2))]).cpu().tolist()
            else:
                xh = ((x.double() - xmu.double()) * xis.double()).abs()
                row["mag"] = torch.cat([o.abs().sum((0, 1, 2)), (o.abs() * xh).sum((0, 1, 2))]).cpu().tolist()
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
        print("%-5s %2dx%3d^2x%-4d %-6s %s" % (kind, B, hw, c, var, " ".join("%.1f" % t for t in times)), flush=True)
        del sets, keep
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(res, f)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def compare(base, new):
    bad = False
    print("%-5s %-14s %-6s %8s | %8s %6s | %8s %6s | %5s  %s" % ("", "shape", "var", "MB", "base us", "spread", "new us", "spread",
                                                                "ratio", "outputs"))
    for rb, rn in zip(base["rows"], new["rows"]):
        assert [rb[k] for k in ("kind", "B", "hw", "c", "var")] == [rn[k] for k in ("kind", "B", "hw", "c", "var")]
        same = rb["out"] == rn["out"] and rb.get("slabs") == rn.get("slabs")
        what = {"fwd": "y", "dgrad": "dx", "bwd": "dx, slabs"}[rb["kind"]] + (" bit-identical" if same else " DIFFERENT")
        if "sums" in rb:
            err = max(abs(x - y) / max(m, 1e-30) for x, y, m in zip(rb["sums"], rn["sums"], rb["mag"]))
            same = same and err < SUM_BOUND
            what += "; %s within %.1e (bound %.0e)" % ("statistics" if rb["kind"] == "fwd" else "BN(x) sums", err, SUM_BOUND)
        mb_, mn = median(rb["us"]), median(rn["us"])
        sb, sn = max(rb["us"]) - min(rb["us"]), max(rn["us"]) - min(rn["us"])
        slower = mn - mb_ > sb
        bad = bad or slower or not same
        print("%-5s %2dx%3dx%3dx%-4d %-6s %8.2f | %8.1f %6.1f | %8.1f %6.1f | %5.2f  %s%s" % (
            rb["kind"], rb["B"], rb["hw"], rb["hw"], rb["c"], rb["var"], rb["mb"], mb_, sb, mn, sn, mb_ / mn, what,
            "  SLOWER" if slower else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base")
    ap.add_argument("--new", default=os.path.join(ROOT, "instance-segmentation-attention_amd", "libisa_kernels.so"))
    ap.add_argument("--out", default="ab_dw_forward_out")
    ap.add_argument("--limit", type=int, default=240, help="seconds per build")
    ap.add_argument("--compare", action="store_true", help="only compare the two result files already in --out")
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    if a.compare:
        return compare(*[json.load(open(os.path.join(a.out, "ab_dw_forward_%s.json" % t))) for t in ("base", "new")])
    if not a.base:
        ap.error("--base is required")
    os.makedirs(a.out, exist_ok=True)
    files = []
    for tag, path in (("base", a.base), ("new", a.new)):
        out = os.path.join(a.out, "ab_dw_forward_%s.json" % tag)
        env = dict(os.environ, ISA_KERNELS_LIB=os.path.abspath(path))
        print("== %s: %s" % (tag, path), flush=True)
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", out], env=env)
        if rc != 0:                      # a fault, an abort or the time limit: nothing more starts on the GPU
            print("%s build ended with status %d" % (tag, rc))
            return rc
        files.append(out)
    return compare(*[json.load(open(f)) for f in files])


if __name__ == "__main__":
    sys.exit(main())
