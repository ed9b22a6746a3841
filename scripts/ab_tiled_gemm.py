#!/usr/bin/env python3
"""A/B of the LDS-tiled small GEMM (conv_gemm_tiled_kernel behind isa_conv_gemm) between two builds of the kernel
library: is y bit-identical, do the statistics agree, and what is the device time of a launch on HBM-cold operands.

    python scripts/ab_tiled_gemm.py --base PATH/libisa_kernels.so [--new PATH/libisa_kernels.so] [--out DIR]
    python scripts/ab_tiled_gemm.py --compare [--out DIR]          (the table again, from the two result files)

Modelled on scripts/ab_fixed_cost.py: --base is a build of the commit to compare against, --new defaults to the library
in the tree; each build runs in a process of its own (ISA_KERNELS_LIB selects it) under its own time limit, the second
starts only if the first ended well, and this process never touches the GPU.

Rows: low-resolution 1x1 shapes of a 256x256, batch 16, bf16 training step (32 images at 16x16 and 32x32 after the decoder
iterations are batched; channel pairs whose bytes are the 12.6 / 25.2 / 50.3 MB rows of
profiles/pw_recompute_step_shapes.txt, and 1024 -> 1024 at 16x16), forward (ReLU6 prologue, statistics) and data gradient
(no prologue, accumulate), and the tiny shapes of tests/test_gpu_tiled_gemm.py.  Inputs are seeded, so both builds see
the same bits.  Per row:
  * y must be bit-identical between the builds;
  * the statistics (float atomics into 8 replicas, unordered in both builds) must agree within SUM_BOUND = 1e-5 of their
    sums of |terms|;
  * time: the operand sets rotate so that no launch finds its inputs in the 256 MB Infinity Cache; REPEATS event-timed
    loops give the median and the spread (max - min) of each build.
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
# images, h = w, K, N, variant: "fwd" (ReLU6 prologue, bias, statistics), "fwd+bs" (with a per-image multiplier),
# "dgrad" (no prologue, accumulate into y), "plain" (no prologue, bias, statistics)
ROWS = [(32, 16, 256, 512, "fwd"), (32, 16, 512, 256, "dgrad"), (32, 16, 512, 1024, "fwd"), (32, 16, 1024, 512, "dgrad"),
        (32, 16, 1024, 1024, "fwd"), (32, 16, 1024, 1024, "dgrad"), (32, 32, 128, 256, "fwd"), (32, 32, 256, 128, "dgrad"),
        (32, 32, 256, 512, "fwd"), (32, 32, 512, 256, "dgrad"), (32, 32, 256, 512, "plain"), (32, 16, 512, 1024, "fwd+bs"),
        (3, 10, 128, 64, "plain"), (3, 10, 320, 64, "fwd"), (3, 10, 2048, 64, "fwd"), (1, 1, 128, 64, "fwd"),
        (3, 7, 320, 80, "fwd+bs"), (3, 7, 192, 144, "dgrad"), (2, 64, 320, 1024, "fwd"), (2, 64, 1024, 1024, "fwd"),
        (2, 64, 128, 1040, "plain")]


def worker(out_path):
    sys.path[:0] = [ROOT]
    import torch
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    lib = L.lib()
    st = L.stream_ptr()
    bf = torch.bfloat16
    res = {"lib": L.LIB_PATH, "rows": []}
    for B, hw, K, N, var in ROWS:
        M = B * hw * hw
        gen = torch.Generator(device="cuda").manual_seed(11 + N + 3 * K + hw)
        nsets = max(2, min(24, -(-(640 << 20) // (M * (K + N) * 2))))

        def tens(c, scale=1.0):
            return (torch.randn(B, hw, hw, c, device="cuda", generator=gen) * scale).to(bf)

        def desc(t):
            return L.IsaTensor(t.data_ptr(), B, hw, hw, t.shape[3], t.shape[3], L.dtype_code(bf), 1)
        W = (torch.randn(N, K, device="cuda", generator=gen) * K ** -0.5).to(bf).contiguous()
        bias = torch.randn(N, device="cuda", generator=gen)
        sc = torch.rand(K, device="cuda", generator=gen) + 0.5
        sh = torch.rand(K, device="cuda", generator=gen) - 0.5
        mask = ((torch.rand(B, K, device="cuda", generator=gen) > 0.2).float() * 1.25).contiguous()
        pro = None
        if var.startswith("fwd"):
            pro = L.IsaPro(L.addr(sc), L.addr(sh), L.addr(mask) if var.endswith("+bs") else None, L.ACT_RELU6, None)
        dgrad = var == "dgrad"
        stats = None if dgrad else torch.zeros(8 * 2 * N, device="cuda")
        sets, keep = [], []
        for _ in range(nsets):
            x, y = tens(K, 2.0), tens(N)
            d = [desc(x), desc(y)]
            keep.append((d, x, y))
            fn = (lambda d=d: lib.isa_conv_gemm(C.byref(d[0]), C.byref(pro) if pro else None, L.ptr(W), K,
                                                None if dgrad else L.ptr(bias), C.byref(d[1]), L.IN_1X1, L.OUT_PLAIN,
                                                L.ptr(stats) if stats is not None else None, int(dgrad), st))
            sets.append((fn, y))
        # outputs of one launch on set 0, from the seeded inputs
        fn, y = sets[0]
        L.check(fn(), var)
        torch.cuda.synchronize()
        row = {"B": B, "hw": hw, "K": K, "N": N, "var": var, "nsets": nsets, "mb": M * (K + N) * 2 / 1e6,
               "y": hashlib.sha256(y.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()}
        if stats is not None:
            row["sums"] = stats.view(8, 2 * N).double().sum(0).cpu().tolist()
            a = y.double().abs().sum((0, 1, 2))                      # the stored y stands in for the fp32 terms (magnitudes only)
            row["mag"] = torch.cat([a, (y.double() ** 2).sum((0, 1, 2))]).cpu().tolist()
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
        print("%2dx%3d^2 %4d->%-4d %-7s %s" % (B, hw, K, N, var, " ".join("%.1f" % t for t in times)), flush=True)
        del sets, keep
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(res, f)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def compare(base, new):
    bad = False
    print("%-10s %-11s %-7s %7s | %8s %6s | %8s %6s | %5s  %s" % ("pixels", "K -> N", "variant", "MB", "base us", "spread", "new us",
                                                                "spread", "ratio", "outputs"))
    for rb, rn in zip(base["rows"], new["rows"]):
        assert [rb[k] for k in ("B", "hw", "K", "N", "var")] == [rn[k] for k in ("B", "hw", "K", "N", "var")]
        same = rb["y"] == rn["y"]
        what = "y bit-identical" if same else "y DIFFERENT"
        if "sums" in rb:
            err = max(abs(x - y) / max(m, 1e-30) for x, y, m in zip(rb["sums"], rn["sums"], rb["mag"]))
            same = same and err < SUM_BOUND
            what += "; statistics within %.1e (bound %.0e)" % (err, SUM_BOUND)
        mb_, mn = median(rb["us"]), median(rn["us"])
        sb, sn = max(rb["us"]) - min(rb["us"]), max(rn["us"]) - min(rn["us"])
        slower = mn - mb_ > sb
        bad = bad or slower or not same
        print("%2dx%3dx%-3d %4d->%-5d %-7s %7.2f | %8.1f %6.1f | %8.1f %6.1f | %5.2f  %s%s" % (
            rb["B"], rb["hw"], rb["hw"], rb["K"], rb["N"], rb["var"], rb["mb"], mb_, sb, mn, sn, mb_ / mn, what,
            "  SLOWER" if slower else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base")
    ap.add_argument("--new", default=os.path.join(ROOT, "instance-segmentation-attention_amd", "libisa_kernels.so"))
    ap.add_argument("--out", default="ab_tiled_gemm_out")
    ap.add_argument("--limit", type=int, default=240, help="seconds per build")
    ap.add_argument("--compare", action="store_true", help="only compare the two result files already in --out")
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    if a.compare:
        return compare(*[json.load(open(os.path.join(a.out, "ab_tiled_gemm_%s.json" % t))) for t in ("base", "new")])
    if not a.base:
        ap.error("--base is required")
    os.makedirs(a.out, exist_ok=True)
    files = []
    for tag, path in (("base", a.base), ("new", a.new)):
        out = os.path.join(a.out, "ab_tiled_gemm_%s.json" % tag)
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
