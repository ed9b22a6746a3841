#!/usr/bin/env python3
"""A/B inside ONE build of the kernel library: the two fused backward entry points for convs WITH a bias
(isa_conv1x1_bias_bn_backward with y = NULL, isa_dwconv3x3_bias_bn_backward) against the separate-kernel sequence they
replace, on HBM-cold operands.

    python scripts/ab_fused_bias.py [--out DIR] [--limit SECONDS]
    python scripts/ab_fused_bias.py --compare [--out DIR]          (the table again, from the result file)

The measuring runs in a child process under a time limit; this process never touches the GPU.  (The form of
scripts/ab_pw_recompute.py.)

Rows: the five convs of the instance stems at a 256x256, batch 16, bf16 training step (depthwise 32, 1x1 32 -> 24,
1x1 24 -> 48, depthwise 48, 1x1 48 -> 24, each with the prologue and the BN(x) sums it has there) and tiny shapes, where a
launch is nothing but its prologue and its fold.  The separate side is what Engine runs with ISA_FUSE_BIAS=0:
isa_bn_bwd_apply, the weight gradient (isa_conv_wgrad / isa_dwconv3x3_wgrad, with dbias), the data gradient
(isa_conv_gemm / isa_dwconv3x3_dgrad) and, where the fused call produces the BN(x) sums, isa_bn_bwd_reduce.
A third column times the bias-free entry points (isa_conv1x1_bn_backward, isa_dwconv3x3_bn_backward) on the same operands:
what the bias sum costs inside the fused launch.
Time: the operand sets rotate so that no launch finds its inputs in the 256 MB Infinity Cache; REPEATS event-timed loops
per side, the sides alternating, give the median and the spread (max - min) of each.  The 1x1 rows also state the worst
|dbias(fused) - dbias(separate)| in units of sum |dy| (bound 2**-8, tests/test_gpu_fused_bias_pw.py).
Exit status 1 when a row's fused median exceeds the separate median.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS = 5
# kind, N (out), K (in), images, h = w, xmode (0 plain x, 1 ReLU6 prologue + BN(x) sums), addend, BN(y) activation
ROWS = [("dw", 32, 32, 16, 256, 0, 0, "relu6"), ("pw", 24, 32, 16, 256, 1, 0, "relu6"), ("pw", 48, 24, 16, 256, 0, 1, "relu6"),
        ("dw", 48, 48, 16, 256, 1, 0, "relu6"), ("pw", 24, 48, 16, 256, 1, 0, "none"),
        ("dw", 32, 32, 2, 8, 0, 0, "relu6"), ("pw", 24, 32, 2, 8, 1, 0, "relu6"), ("dw", 48, 48, 16, 32, 1, 0, "relu6"),
        ("pw", 24, 48, 16, 32, 1, 0, "none")]


def worker(out_path):
    sys.path[:0] = [ROOT]
    import torch
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    lib = L.checked()
    st = L.stream_ptr()
    bf = torch.bfloat16
    ws = torch.zeros(16 << 20, device="cuda")
    res = {"lib": L.LIB_PATH, "rows": []}
    for kind, N, K, B, hw, xmode, epi, yact_name in ROWS:
        M = B * hw * hw
        yact = L.ACT_RELU6 if yact_name == "relu6" else L.ACT_NONE
        gen = torch.Generator(device="cuda").manual_seed(7 + N + 3 * K + hw)
        nsets = max(2, min(24, -(-(640 << 20) // (5 * M * max(N, K) * 2))))

        def tens(c, scale=1.0):
            return (torch.randn(B, hw, hw, c, device="cuda", generator=gen) * scale).to(bf)

        def desc(t):
            return L.IsaTensor(t.data_ptr(), B, hw, hw, t.shape[3], t.shape[3], L.dtype_code(bf), 1)

        def vec(c, lo=0.5):
            return (torch.rand(c, device="cuda", generator=gen) + lo).contiguous()
        ysc, ysh, ymu, yis, gam = vec(N), vec(N, -0.5), vec(N, -0.5), vec(N), vec(N)
        yred = torch.zeros(8 * 2 * N, device="cuda")
        yred[:2 * N] = torch.randn(2 * N, device="cuda", generator=gen) * M * 0.01
        xsc, xsh, xmu, xis = vec(K), vec(K, -0.5), vec(K, 0.0), vec(K)
        dgam, dbet = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        bias = (torch.randn(N, device="cuda", generator=gen) * 0.5).contiguous()
        db = {s: torch.zeros(N, device="cuda") for s in ("fused", "separate")}
        xpro = L.IsaPro(L.addr(xsc), L.addr(xsh), None, L.ACT_RELU6, None)
        pro = C.byref(xpro) if xmode else None
        ybn = L.IsaBnBwd(L.addr(ysc), L.addr(ysh), L.addr(ymu), L.addr(yis), L.addr(yred), None, L.addr(dgam), L.addr(dbet),
                         float(M), yact)
        if kind == "pw":
            W = (torch.randn(N, K, device="cuda", generator=gen) * K ** -0.5).contiguous()
            dw = torch.zeros(N, K, device="cuda")
            kp, kpd = (K + 31) // 32 * 32, (N + 31) // 32 * 32
            Wp = torch.zeros(N, kp, device="cuda", dtype=bf)
            Wp[:, :K] = W.to(bf)
            Wd = torch.zeros(K, kpd, device="cuda", dtype=bf)           # data-gradient packing: W^T, rows padded to 32
            Wd[:, :N] = W.t().to(bf)
        else:
            Wf = (torch.randn(9, (N + 7) // 8 * 8, device="cuda", generator=gen) / 3).to(bf).contiguous()       # tap-major packing
            dw = torch.zeros(N, 9, device="cuda")
        sets, keep = [], []
        for _ in range(nsets):
            g, x, dx, dy = tens(N), tens(K, 2.0), tens(K), tens(N)
            y = torch.empty(B, hw, hw, N, device="cuda", dtype=bf)
            add = tens(K) if epi else None
            xred = torch.zeros(8 * 2 * K, device="cuda")
            xbn = L.IsaBnBwd(L.addr(xsc), L.addr(xsh), L.addr(xmu), L.addr(xis), None, L.addr(xred), None, None, 1.0, 0)
            d = dict(g=desc(g), y=desc(y), x=desc(x), dx=desc(dx), dy=desc(dy), add=desc(add) if epi else None)
            if kind == "pw":
                lib.isa_conv_gemm(C.byref(d["x"]), pro, L.ptr(Wp), kp, L.ptr(bias), C.byref(d["y"]), L.IN_1X1, L.OUT_PLAIN, None, 0, st)
            else:
                lib.isa_dwconv3x3(C.byref(d["x"]), pro, L.ptr(Wf), L.ptr(bias), C.byref(d["y"]), None, st)
            keep.append((xbn, d, g, y, x, dx, dy, add, xred))
            addp = C.byref(d["add"]) if epi else None

            def fused(d=d, xbn=xbn, addp=addp):
                xb = C.byref(xbn) if xmode else None
                if kind == "pw":
                    lib.isa_conv1x1_bias_bn_backward(C.byref(d["g"]), None, C.byref(ybn), C.byref(d["x"]), pro, xb, L.ptr(W), L.ptr(dw),
                                                     C.byref(d["dx"]), 0, addp, L.ptr(ws), ws.numel(), None, st, L.ptr(bias),
                                                     L.ptr(db["fused"]))
                else:
                    lib.isa_dwconv3x3_bias_bn_backward(C.byref(d["g"]), C.byref(d["y"]), C.byref(ybn), C.byref(d["x"]), pro, xb, L.ptr(Wf),
                                                       L.ptr(dw), N, C.byref(d["dx"]), 0, addp, L.ptr(ws), ws.numel(), None, st,
                                                       L.ptr(db["fused"]))

            def nobias(d=d, xbn=xbn, addp=addp):
                xb = C.byref(xbn) if xmode else None
                if kind == "pw":
                    lib.isa_conv1x1_bn_backward(C.byref(d["g"]), None, C.byref(ybn), C.byref(d["x"]), pro, xb, L.ptr(W), L.ptr(dw),
                                                C.byref(d["dx"]), 0, addp, L.ptr(ws), ws.numel(), None, st)
                else:
                    lib.isa_dwconv3x3_bn_backward(C.byref(d["g"]), C.byref(d["y"]), C.byref(ybn), C.byref(d["x"]), pro, xb, L.ptr(Wf),
                                                  L.ptr(dw), N, C.byref(d["dx"]), 0, addp, L.ptr(ws), ws.numel(), None, st)

            def separate(d=d, xred=xred, addp=addp):
                lib.isa_bn_bwd_apply(C.byref(d["g"]), C.byref(d["y"]), ysc, ysh, ymu, yis, yact, None, L.ptr(gam), yred, float(M), 1,
                                     C.byref(d["dy"]), L.ptr(dgam), L.ptr(dbet), st)
                if kind == "pw":
                    lib.isa_conv_wgrad(C.byref(d["x"]), pro, C.byref(d["dy"]), L.ptr(dw), L.ptr(db["separate"]), L.IN_1X1, L.OUT_PLAIN,
                                       None, K, L.ptr(ws), ws.numel(), None, st)
                    lib.isa_conv_gemm(C.byref(d["dy"]), None, L.ptr(Wd), kpd, None, C.byref(d["dx"]), L.IN_1X1, L.OUT_PLAIN, None, 0, st)
                else:
                    lib.isa_dwconv3x3_wgrad(C.byref(d["x"]), pro, C.byref(d["dy"]), L.ptr(dw), L.ptr(db["separate"]), N, L.ptr(ws),
                                            ws.numel(), None, st)
                    lib.isa_dwconv3x3_dgrad(C.byref(d["dy"]), L.ptr(Wf), C.byref(d["dx"]), 0, st)
                if epi:
                    lib.isa_axpy(C.byref(d["add"]), C.byref(d["dx"]), 1.0, 1, st)
                if xmode:
                    lib.isa_bn_bwd_reduce(C.byref(d["dx"]), C.byref(d["x"]), xsc, xsh, xmu, xis, L.ACT_RELU6, None, xred, st)
            sets.append(dict(fused=fused, separate=separate, nobias=nobias, dy=dy))
        torch.cuda.synchronize()
        row = {"kind": kind, "N": N, "K": K, "B": B, "hw": hw, "var": [xmode, epi], "yact": yact_name, "nsets": nsets,
               "launches": 3 + epi + xmode}
        # bytes each side moves: fused reads g, x (+ y for the depthwise), writes dx (+ addend); separate: apply 3 N,
        # weight gradient N + K, data gradient N + K (+ 3 K addend) (+ 2 K reduce)
        row["fused"] = {"mb": M * ((1 if kind == "pw" else 2) * N + (2 + epi) * K) * 2 / 1e6, "us": []}
        row["separate"] = {"mb": M * (5 * N + (2 + 3 * epi + 2 * xmode) * K) * 2 / 1e6, "us": []}
        row["nobias"] = {"us": []}
        # the bias gradients of one launch of each side on set 0
        for side in ("fused", "separate"):
            db[side].zero_()
            sets[0][side]()
        torch.cuda.synchronize()
        mag = sets[0]["dy"].double().abs().sum((0, 1, 2)).clamp_min(1e-30)
        row["dbias_err"] = float(((db["fused"].double() - db["separate"].double()).abs() / mag).max())
        loops = max(2, 48 // nsets)
        for side in ("fused", "separate", "nobias"):
            for f in sets:
                f[side]()
        torch.cuda.synchronize()
        for _ in range(REPEATS):
            for side in ("separate", "fused", "nobias"):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(loops):
                    for f in sets:
                        f[side]()
                e.record()
                torch.cuda.synchronize()
                row[side]["us"].append(s.elapsed_time(e) * 1e3 / (loops * nsets))
        res["rows"].append(row)
        print("%s %3dx%-3d %2dx%3d^2 separate %s | fused %s | bias-free %s" % (
            kind, N, K, B, hw, *(" ".join("%.1f" % t for t in row[s]["us"]) for s in ("separate", "fused", "nobias"))), flush=True)
        del sets, keep
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(res, f)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def compare(res):
    bad = False
    print("%-4s %-8s %-10s %-6s %-5s | %2s %7s %8s %6s | %7s %8s %6s %6s | %9s | %5s  %s" % (
        "kind", "N x K", "pixels", "var", "yact", "n", "MB", "sep us", "spread", "MB", "fused us", "spread", "GB/s", "bias-free", "ratio", "dbias"))
    for r in res["rows"]:
        a, b = r["separate"], r["fused"]
        ma, mb = median(a["us"]), median(b["us"])
        sa, sb = max(a["us"]) - min(a["us"]), max(b["us"]) - min(b["us"])
        slower = mb > ma
        bad = bad or slower
        print("%-4s %3dx%-4d %2dx%3dx%-3d %-6s %-5s | %2d %7.2f %8.1f %6.1f | %7.2f %8.1f %6.1f %6.0f | %9.1f | %5.2f  %.1e of sum |dy|%s" % (
            r["kind"], r["N"], r["K"], r["B"], r["hw"], r["hw"], tuple(r["var"]), r["yact"], r["launches"], a["mb"], ma, sa,
            b["mb"], mb, sb, b["mb"] / mb * 1e3, median(r["nobias"]["us"]), ma / mb, r["dbias_err"], "  SLOWER" if slower else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="ab_fused_bias_out")
    ap.add_argument("--limit", type=int, default=300, help="seconds for the measuring process")
    ap.add_argument("--compare", action="store_true", help="only print the table of the result file already in --out")
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    out = os.path.join(a.out, "ab_fused_bias.json")
    if not a.compare:
        os.makedirs(a.out, exist_ok=True)
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", out])
        if rc != 0:                      # a fault, an abort or the time limit: nothing more starts on the GPU
            print("the measuring process ended with status %d" % rc)
            return rc
    return compare(json.load(open(out)))


if __name__ == "__main__":
    sys.exit(main())
