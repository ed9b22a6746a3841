#!/usr/bin/env python3
"""A/B of isa_conv1x1_bn_backward inside ONE build of the kernel library: the call with the stored conv output y against
the call with y = NULL (the kernel recomputes y from pro(x) and W).  Are the outputs bit-identical, and what is the device
time of a launch on HBM-cold operands.

    python scripts/ab_pw_recompute.py [--out DIR] [--limit SECONDS]
    python scripts/ab_pw_recompute.py --compare [--out DIR]          (the table again, from the result file)

The measuring runs in a child process under a time limit; this process never touches the GPU.  (Modelled on
scripts/ab_fixed_cost.py.)

Rows: every isa_conv1x1_bn_backward shape of a 256x256, batch 16, bf16 training step (profiles/dw_pipeline_step_shapes.txt:
the 805 / 402 / 268 / 201 MB launches, i.e. 64 <-> 32 channels over 32 images at 256^2 and 128^2 and over 16 images at
256^2, 32 -> 32 over 16 images at 256^2) and the tiny shapes of profiles/fixed_cost_floors.txt (64 -> 64 channels, 16 images
at 8^2 / 32^2 / 64^2) and of tests/test_gpu_fixed_cost.py, where a launch is nothing but its prologue and its fold.  Per row:
  * y of every operand set is produced by the forward kernel (isa_conv_gemm: 1x1, plain output, the same prologue and the
    bf16 packing of the same W), which is what the y = NULL call assumes;
  * dx and the partial slabs must be bit-identical between the two calls, the BN(x) sums (float atomics into 8 replicas)
    within SUM_BOUND = 1e-5 of their sums of |terms|;
  * time: the operand sets rotate so that no launch finds its inputs in the 256 MB Infinity Cache; REPEATS event-timed
    loops per side, the sides alternating, give the median and the spread (max - min) of each.  The time is that of the
    entry point: kernel plus second-stage reduce.  MB and GB/s count what the call moves: g, x and (stored side) y read,
    dx written, old dx and addend read with the epilogue.
Exit status 1 when an output differs, or when a row's y = NULL median exceeds the stored-y median by more than the
stored side's spread.
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
# N, K, images, h = w, (xmode: 0 plain x, 1 ReLU6 prologue + BN(x) sums; epi), BN(y) activation
ROWS = [(64, 32, 32, 256, (1, 0), "relu6"), (32, 64, 32, 256, (1, 1), "none"), (64, 32, 16, 256, (1, 0), "relu6"),
        (32, 64, 16, 256, (1, 0), "none"), (32, 32, 16, 256, (1, 0), "none"), (64, 32, 32, 128, (1, 0), "relu6"),
        (32, 64, 32, 128, (1, 1), "none"), (64, 64, 16, 64, (1, 0), "relu6"), (64, 64, 16, 32, (1, 0), "relu6"),
        (64, 64, 16, 8, (1, 0), "relu6"), (8, 8, 2, 4, (1, 0), "relu6"), (24, 40, 1, 8, (1, 1), "none"),
        (64, 64, 1, 1, (1, 0), "relu6")]


def slab_floats(N, K, M):
    nt, kt = (N + 31) // 32, (K + 31) // 32
    return min(((M + 31) // 32 + 3) // 4, 512) * (nt * kt * 1024 + nt * 32)


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
    for N, K, B, hw, (xmode, epi), yact_name in ROWS:
        M = B * hw * hw
        yact = L.ACT_RELU6 if yact_name == "relu6" else L.ACT_NONE
        gen = torch.Generator(device="cuda").manual_seed(7 + N + 3 * K + hw)
        nsets = max(2, min(24, -(-(640 << 20) // (4 * M * max(N, K) * 2))))

        def tens(c, scale=1.0, offset=0.0):
            return (torch.randn(B, hw, hw, c, device="cuda", generator=gen) * scale + offset).to(bf)

        def desc(t):
            return L.IsaTensor(t.data_ptr(), B, hw, hw, t.shape[3], t.shape[3], L.dtype_code(bf), 1)

        def vec(c, lo=0.5):
            return (torch.rand(c, device="cuda", generator=gen) + lo).contiguous()
        W = (torch.randn(N, K, device="cuda", generator=gen) * K ** -0.5).contiguous()
        kp = (K + 31) // 32 * 32
        Wp = torch.zeros(N, kp, device="cuda", dtype=bf)
        Wp[:, :K] = W.to(bf)
        ysc, ysh, ymu, yis = vec(N), vec(N, -0.5), vec(N, -0.5), vec(N)
        yred = torch.zeros(8 * 2 * N, device="cuda")
        yred[:2 * N] = torch.randn(2 * N, device="cuda", generator=gen) * M * 0.01
        xsc, xsh, xmu, xis = vec(K), vec(K, -0.5), vec(K, 0.0), vec(K)
        dgam, dbet = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        dw = torch.zeros(N, K, device="cuda")
        xpro = L.IsaPro(L.addr(xsc), L.addr(xsh), None, L.ACT_RELU6, None)
        ybn = L.IsaBnBwd(L.addr(ysc), L.addr(ysh), L.addr(ymu), L.addr(yis), L.addr(yred), None, L.addr(dgam), L.addr(dbet),
                         float(M), yact)
        sets, keep = [], []
        for _ in range(nsets):
            g, x, dx = tens(N), tens(K, 2.0), tens(K)
            y = torch.empty(B, hw, hw, N, device="cuda", dtype=bf)
            add = tens(K) if epi else None
            xred = torch.zeros(8 * 2 * K, device="cuda")
            xbn = L.IsaBnBwd(L.addr(xsc), L.addr(xsh), L.addr(xmu), L.addr(xis), None, L.addr(xred), None, None, 1.0, 0)
            d = [desc(g), desc(y), desc(x), desc(dx), desc(add) if epi else None]
            L.check(lib.isa_conv_gemm(C.byref(d[2]), C.byref(xpro) if xmode else None, L.ptr(Wp), kp, None, C.byref(d[1]), L.IN_1X1,
                                      L.OUT_PLAIN, None, 0, st), "isa_conv_gemm")
            keep.append((xbn, d, g, y, x, add))

            def fn(with_y, d=d, xbn=xbn):
                return lib.isa_conv1x1_bn_backward(
                    C.byref(d[0]), C.byref(d[1]) if with_y else None, C.byref(ybn), C.byref(d[2]), C.byref(xpro) if xmode else None,
                    C.byref(xbn) if xmode else None, L.ptr(W), L.ptr(dw), C.byref(d[3]), int(epi),
                    C.byref(d[4]) if epi else None, L.ptr(ws), ws.numel(), None, st)
            sets.append((fn, dx, xred, x))
        torch.cuda.synchronize()

        def sha(t):
            return hashlib.sha256(t.contiguous().view(torch.int16 if t.dtype == bf else torch.int32).cpu().numpy().tobytes()).hexdigest()
        # outputs of one launch of each side on set 0, from the same inputs (the epilogue accumulates into dx: restored between)
        fn, dx, xred, x = sets[0]
        dx0 = dx.clone()
        row = {"N": N, "K": K, "B": B, "hw": hw, "var": [xmode, epi], "yact": yact_name, "nsets": nsets}
        for side, with_y in (("stored", True), ("null", False)):
            dx.copy_(dx0)
            xred.zero_()
            L.check(fn(with_y), "isa_conv1x1_bn_backward")
            torch.cuda.synchronize()
            o = {"dx": sha(dx), "slabs": sha(ws[:slab_floats(N, K, M)]),
                 "mb": M * ((2 if with_y else 1) * N + (2 + 2 * epi) * K) * 2 / 1e6}
            if xmode:
                o["sums"] = xred.view(8, 2 * K).double().sum(0).cpu().tolist()
                a = dx.double().abs().sum((0, 1, 2))
                xh = ((x.double() - xmu.double()) * xis.double()).abs()
                o["mag"] = torch.cat([a, (dx.double().abs() * xh).sum((0, 1, 2))]).cpu().tolist()
            row[side] = o
        # timing: every launch on the next operand set, the two sides alternating
        loops = max(2, 96 // nsets)
        for side in ("stored", "null"):
            row[side]["us"] = []
        for with_y in (True, False):
            for f in sets:
                f[0](with_y)
        torch.cuda.synchronize()
        for _ in range(REPEATS):
            for side, with_y in (("stored", True), ("null", False)):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(loops):
                    for f in sets:
                        f[0](with_y)
                e.record()
                torch.cuda.synchronize()
                row[side]["us"].append(s.elapsed_time(e) * 1e3 / (loops * nsets))
        res["rows"].append(row)
        print("%3dx%-3d %2dx%3d^2 %s %-5s stored %s | null %s" % (N, K, B, hw, (xmode, epi), yact_name,
                                                                " ".join("%.1f" % t for t in row["stored"]["us"]),
                                                                " ".join("%.1f" % t for t in row["null"]["us"])), flush=True)
        del sets, keep
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(res, f)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def compare(res):
    bad = False
    print("%-8s %-10s %-6s %-5s | %7s %8s %6s %6s | %7s %8s %6s %6s | %5s  %s" % (
        "N x K", "pixels", "var", "yact", "MB", "y us", "spread", "GB/s", "MB", "NULL us", "spread", "GB/s", "ratio", "outputs"))
    for r in res["rows"]:
        a, b = r["stored"], r["null"]
        same = a["dx"] == b["dx"] and a["slabs"] == b["slabs"]
        what = "dx, slabs" + (" bit-identical" if same else " DIFFERENT")
        if "sums" in a:
            err = max(abs(x - y) / max(m, 1e-30) for x, y, m in zip(a["sums"], b["sums"], a["mag"]))
            same = same and err < SUM_BOUND
            what += "; BN(x) sums within %.1e (bound %.0e)" % (err, SUM_BOUND)
        ma, mb = median(a["us"]), median(b["us"])
        sa, sb = max(a["us"]) - min(a["us"]), max(b["us"]) - min(b["us"])
        slower = mb - ma > sa
        bad = bad or slower or not same
        print("%3dx%-4d %2dx%3dx%-3d %-6s %-5s | %7.2f %8.1f %6.1f %6.0f | %7.2f %8.1f %6.1f %6.0f | %5.2f  %s%s" % (
            r["N"], r["K"], r["B"], r["hw"], r["hw"], tuple(r["var"]), r["yact"], a["mb"], ma, sa, a["mb"] / ma * 1e3,
            b["mb"], mb, sb, b["mb"] / mb * 1e3, ma / mb, what, "  SLOWER" if slower else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="ab_pw_recompute_out")
    ap.add_argument("--limit", type=int, default=300, help="seconds for the measuring process")
    ap.add_argument("--compare", action="store_true", help="only print the table of the result file already in --out")
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    out = os.path.join(a.out, "ab_pw_recompute.json")
    if not a.compare:
        os.makedirs(a.out, exist_ok=True)
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", out])
        if rc != 0:                      # a fault, an abort or the time limit: nothing more starts on the GPU
            print("the measuring process ended with status %d" % rc)
            return rc
    return compare(json.load(open(out)))


if __name__ == "__main__":
    sys.exit(main())
