#!/usr/bin/env python3
"""A/B of the wave-private MFMA backward kernels (isa_conv1x1_bn_backward, bf16 isa_conv_wgrad) between two builds of
the kernel library: are the outputs bit-identical, and what is the device time of a launch on HBM-cold operands.

    python scripts/ab_fixed_cost.py --base PATH/libisa_kernels.so [--new PATH/libisa_kernels.so] [--out DIR]
    python scripts/ab_fixed_cost.py --compare [--out DIR]          (the table again, from the two result files)

--base is a build of the commit to compare against, --new defaults to the library in the tree.  Each build runs in a
process of its own (ISA_KERNELS_LIB selects it), under its own time limit; the second starts only if the first ended
well.  This process never touches the GPU.  (Modelled on scripts/ab_streaming.py.)

Rows: the 1x1 shapes of a 256x256, batch 16, bf16 training step (profiles/streaming_step_shapes.txt: the 805 / 402 /
201 MB launches of isa_conv1x1_bn_backward, the 50 / 25 / 12.6 MB launches of isa_conv_wgrad) and the tiny shapes of
tests/test_gpu_fixed_cost.py, where a launch is nothing but its prologue and its fold.  Inputs are seeded, so both
builds see the same bits.  Per row:
  * dx and the partial slabs (what the kernel itself writes: one slab per workgroup, summed over its four waves in the
    order wave 0..3, with the column sums of dy for the bias gradient in the slab tails) must be bit-identical between
    the builds.  dW and the bias gradient, which the second-stage reduce adds with `rsplit` float atomics per address,
    are bit-identical whenever at most two adders share an address and are reported (max difference relative to
    max |dW|, "db identical" or not) otherwise: those atomics are unordered in both builds;
  * the BN(x) sums (float atomics into 8 replicas, unordered in both builds) must agree within SUM_BOUND = 1e-5 of
    their sums of |terms|;
  * time: the operand sets rotate so that no launch finds its inputs in the 256 MB Infinity Cache (KBENCH_ROTATE in
    scripts/kbench.py); REPEATS event-timed loops give the median and the spread (max - min) of each build.  The time
    is that of the entry point: kernel plus second-stage reduce.
Exit status 1 when an output differs, or when a row's new median exceeds the base median by more than the base spread.
"""
import argparse
import base64
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM_BOUND = 1e-5
REPEATS = 5
# kind, N, K, images, h = w, variant.  pw variants: xmode (0 plain x, 1 ReLU6 prologue + BN(x) sums), epi;
# wg variants: prologue form
ROWS = [("pw", 32, 64, 16, 256, (1, 0)), ("pw", 64, 32, 16, 256, (0, 0)), ("pw", 64, 32, 16, 128, (1, 0)),
        ("pw", 32, 64, 16, 128, (1, 1)), ("pw", 64, 64, 16, 128, (1, 0)), ("pw", 64, 32, 32, 64, (1, 0)),
        ("pw", 32, 64, 32, 64, (0, 1)), ("pw", 8, 8, 2, 4, (1, 0)), ("pw", 24, 40, 1, 8, (1, 1)), ("pw", 64, 64, 1, 1, (1, 0)),
        ("wg", 512, 512, 32, 16, "relu6"), ("wg", 512, 512, 32, 16, "none"), ("wg", 256, 256, 32, 32, "relu6"),
        ("wg", 256, 256, 32, 32, "none"), ("wg", 128, 96, 16, 64, "relu6"), ("wg", 512, 256, 16, 16, "relu6+bs"),
        ("wg", 8, 8, 1, 1, "relu6"), ("wg", 40, 24, 3, 11, "relu6+bs"), ("wg", 128, 96, 1, 6, "none")]


def slab_floats(kind, N, K, M):
    """Floats of partial slabs the launch writes (conv_fused_bwd.hip launch_inst / conv_wgrad.hip launch_wg_bf16)."""
    nt, kt = (N + 31) // 32, (K + 31) // 32
    want = ((M + 31) // 32 + 3) // 4
    if kind == "pw":
        return min(want, 512) * (nt * kt * 1024 + nt * 32)
    if nt == 1:
        tn, tk = 1, (4 if kt >= 4 else (2 if kt >= 2 else 1))
    elif kt == 1:
        tk, tn = 1, (4 if nt >= 4 else (2 if nt >= 2 else 1))
    else:
        tn, tk = 2, 2
    gy = -(-nt // tn) * -(-kt // tk)
    return max(1, min(want, 512 // gy)) * gy * (tn * tk * 1024 + tn * 32)


def worker(out_path):
    sys.path[:0] = [ROOT]
    import torch
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    lib = L.lib()
    st = L.stream_ptr()
    bf = torch.bfloat16
    ws = torch.zeros(16 << 20, device="cuda")
    res = {"lib": L.LIB_PATH, "rows": []}
    for kind, N, K, B, hw, var in ROWS:
        M = B * hw * hw
        gen = torch.Generator(device="cuda").manual_seed(7 + N + 3 * K + hw)
        ntens = 4 if kind == "pw" else 2
        nsets = max(2, min(24, -(-(640 << 20) // (ntens * M * max(N, K) * 2))))

        def tens(c, scale=1.0, offset=0.0):
            return (torch.randn(B, hw, hw, c, device="cuda", generator=gen) * scale + offset).to(bf)

        def desc(t):
            return L.IsaTensor(t.data_ptr(), B, hw, hw, t.shape[3], t.shape[3], L.dtype_code(bf), 1)

        def vec(c, lo=0.5):
            return (torch.rand(c, device="cuda", generator=gen) + lo).contiguous()
        keep = []
        if kind == "pw":
            xmode, epi = var
            W = (torch.randn(N, K, device="cuda", generator=gen) * K ** -0.5).to(bf).float().contiguous()
            ysc, ysh, ymu, yis = vec(N), vec(N, -0.5), vec(N), vec(N)
            yred = torch.zeros(8 * 2 * N, device="cuda")
            yred[:2 * N] = torch.randn(2 * N, device="cuda", generator=gen) * M * 0.01
            xsc, xsh, xmu, xis = vec(K), vec(K, -0.5), vec(K, 0.0), vec(K)
            dgam, dbet = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
            dw = torch.zeros(N, K, device="cuda")
            sets = []
            for _ in range(nsets):
                g, y, x, dx = tens(N), tens(N, 2.0, 1.0), tens(K, 2.0), tens(K)
                add = tens(K) if epi else None
                xred = torch.zeros(8 * 2 * K, device="cuda")
                ybn = L.IsaBnBwd(L.addr(ysc), L.addr(ysh), L.addr(ymu), L.addr(yis), L.addr(yred), None, L.addr(dgam),
                                 L.addr(dbet), float(M), L.ACT_RELU6)
                xbn = L.IsaBnBwd(L.addr(xsc), L.addr(xsh), L.addr(xmu), L.addr(xis), None, L.addr(xred), None, None, 1.0, 0)
                xpro = L.IsaPro(L.addr(xsc), L.addr(xsh), None, L.ACT_RELU6, None)
                d = [desc(g), desc(y), desc(x), desc(dx), desc(add) if epi else None]
                keep.append((ybn, xbn, xpro, d, g, y, x, add))
                fn = (lambda d=d, ybn=ybn, xbn=xbn, xpro=xpro: lib.isa_conv1x1_bn_backward(
                    C.byref(d[0]), C.byref(d[1]), C.byref(ybn), C.byref(d[2]), C.byref(xpro) if xmode else None,
                    C.byref(xbn) if xmode else None, L.ptr(W), L.ptr(dw), C.byref(d[3]), int(epi),
                    C.byref(d[4]) if epi else None, L.ptr(ws), ws.numel(), None, st))
                sets.append((fn, dx, xred, x))
        else:
            sc, sh = vec(K), vec(K, -0.5)
            mask = ((torch.rand(B, K, device="cuda", generator=gen) > 0.2).float() * 1.25).contiguous()
            pro = None if var == "none" else L.IsaPro(L.addr(sc), L.addr(sh), L.addr(mask) if var.endswith("+bs") else None,
                                                       L.ACT_RELU6, None)
            dw, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
            sets = []
            for _ in range(nsets):
                x, dy = tens(K, 2.0), tens(N)
                d = [desc(x), desc(dy)]
                keep.append((d, x, dy))
                fn = (lambda d=d: lib.isa_conv_wgrad(C.byref(d[0]), C.byref(pro) if pro else None, C.byref(d[1]), L.ptr(dw),
                                                     L.ptr(db), L.IN_1X1, L.OUT_PLAIN, None, K, L.ptr(ws), ws.numel(), None, st))
                sets.append((fn, None, None, x))
        # outputs of one launch on set 0, from the seeded inputs
        fn, dx, xred, x = sets[0]
        L.check(fn(), kind)
        torch.cuda.synchronize()

        def sha(t):
            return hashlib.sha256(t.contiguous().view(torch.int16 if t.dtype == bf else torch.int32).cpu().numpy().tobytes()).hexdigest()
        row = {"kind": kind, "N": N, "K": K, "B": B, "hw": hw, "var": var, "nsets": nsets,
               "mb": M * (2 * N + (3 if var[1] else 2) * K) * 2 / 1e6 if kind == "pw" else M * (N + K) * 2 / 1e6,
               "slabs": sha(ws[:slab_floats(kind, N, K, M)]),
               "dw": base64.b64encode(dw.cpu().numpy().tobytes()).decode()}
        if kind == "pw":
            row["dx"] = sha(dx)
            if var[0]:
                row["sums"] = xred.view(8, 2 * K).double().sum(0).cpu().tolist()
                a = dx.double().abs().sum((0, 1, 2))
                xh = ((x.double() - xmu.double()) * xis.double()).abs()
                row["mag"] = torch.cat([a, (dx.double().abs() * xh).sum((0, 1, 2))]).cpu().tolist()
        else:
            row["db"] = sha(db)
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
        print("%-3s %3dx%-3d %2dx%3d^2 %-9s %s" % (kind, N, K, B, hw, var, " ".join("%.1f" % t for t in times)), flush=True)
        del sets, keep
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(res, f)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def compare(base, new):
    import numpy as np
    bad = False
    print("%-3s %-8s %-10s %-9s %7s | %8s %6s | %8s %6s | %5s  %s" % ("", "N x K", "pixels", "variant", "MB", "base us", "spread",
                                                                      "new us", "spread", "ratio", "outputs"))
    for rb, rn in zip(base["rows"], new["rows"]):
        assert [rb[k] for k in ("kind", "N", "K", "B", "hw")] == [rn[k] for k in ("kind", "N", "K", "B", "hw")]
        same = rb["slabs"] == rn["slabs"] and rb.get("dx") == rn.get("dx")
        what = ("dx, slabs" if rb["kind"] == "pw" else "slabs") + (" bit-identical" if same else " DIFFERENT")
        if "db" in rb:
            what += "; db identical" if rb["db"] == rn["db"] else "; db differs (reduce atomics)"
        wb, wn = (np.frombuffer(base64.b64decode(r["dw"]), dtype=np.float32).astype(np.float64) for r in (rb, rn))
        ddw = float(np.abs(wb - wn).max() / (np.abs(wb).max() or 1.0))
        what += "; dW identical" if ddw == 0 else "; dW within %.1e" % ddw
        if "sums" in rb:
            err = max(abs(x - y) / max(m, 1e-30) for x, y, m in zip(rb["sums"], rn["sums"], rb["mag"]))
            same = same and err < SUM_BOUND
            what += "; BN(x) sums within %.1e (bound %.0e)" % (err, SUM_BOUND)
        mb_, mn = median(rb["us"]), median(rn["us"])
        sb, sn = max(rb["us"]) - min(rb["us"]), max(rn["us"]) - min(rn["us"])
        slower = mn - mb_ > sb
        bad = bad or slower or not same
        print("%-3s %3dx%-4d %2dx%3dx%-3d %-9s %7.2f | %8.1f %6.1f | %8.1f %6.1f | %5.2f  %s%s" % (
            rb["kind"], rb["N"], rb["K"], rb["B"], rb["hw"], rb["hw"], rb["var"], rb["mb"], mb_, sb, mn, sn, mb_ / mn, what,
            "  SLOWER" if slower else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base")
    ap.add_argument("--new", default=os.path.join(ROOT, "instance-segmentation-attention_amd", "libisa_kernels.so"))
    ap.add_argument("--out", default="ab_fixed_cost_out")
    ap.add_argument("--limit", type=int, default=240, help="seconds per build")
    ap.add_argument("--compare", action="store_true", help="only compare the two result files already in --out")
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    if a.compare:
        return compare(*[json.load(open(os.path.join(a.out, "ab_fixed_cost_%s.json" % t))) for t in ("base", "new")])
    if not a.base:
        ap.error("--base is required")
    os.makedirs(a.out, exist_ok=True)
    files = []
    for tag, path in (("base", a.base), ("new", a.new)):
        out = os.path.join(a.out, "ab_fixed_cost_%s.json" % tag)
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
