#!/usr/bin/env python3
"""Phase stamps of one workgroup of pw_bn_bwd_kernel and conv_wgrad_bf16_kernel: where a launch spends its time before
and after the pixel loop.  Needs a library whose conv_fused_bwd.hip and conv_wgrad.hip were compiled with
-DISA_PHASE_TRACE (off by default; see tr_lds.hpp): thread 0 of workgroup 0 then takes wall_clock64() stamps (100 MHz)
at the phase boundaries and writes them out at the end of the kernel.

    ISA_KERNELS_LIB=<instrumented build>/libisa_kernels.so python scripts/phase_trace.py

Every launch is measured on HBM-cold operands (a 512 MB fill runs before it, as KBENCH_FLUSH does in scripts/kbench.py);
REPEATS launches per row, the median of each stamp.  Columns: microseconds since kernel entry at which wave 0 of
workgroup 0 passed
  const  the barrier behind the staged constants (pw: W and the BN constants in LDS; wg: the per-lane constants requested)
  frag   the barrier behind the W fragment build (pw only)
  chunk  the first chunk stashed to LDS, i.e. its loads have arrived
  loop   the end of its pixel loop
  sync   the barrier in front of the fold (all four waves have left their loops)
  fold   the fold's last barrier (serial form: the four phases; parallel form: the parked partials)
  slab   the slab stores issued
  end    the BN(x) sums added (pw only); the kernel's last instruction
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS = 7
NAMES = ["entry", "const", "frag", "chunk", "loop", "sync", "fold", "slab", "end"]
PW = [(32, 64, 64), (32, 64, 128), (64, 32, 64), (64, 32, 128)]                      # N, K, h = w; 32 images
WG = [(512, 512, 16, "none"), (512, 512, 16, "relu6"), (512, 512, 32, "none"), (512, 512, 32, "relu6"),
      (256, 256, 16, "none"), (256, 256, 16, "relu6"), (256, 256, 32, "none"), (256, 256, 32, "relu6")]


def main():
    sys.path[:0] = [ROOT]
    import torch
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    lib = L.lib()
    if not hasattr(lib, "isa_phase_trace_pw"):
        sys.exit("%s was not built with -DISA_PHASE_TRACE" % L.LIB_PATH)
    st = L.stream_ptr()
    bf = torch.bfloat16
    B = 32
    ws = torch.zeros(16 << 20, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)
    out = (C.c_ulonglong * 10)()

    def tens(hw, c, scale=1.0):
        return (torch.randn(B, hw, hw, c, device="cuda", generator=gen) * scale).to(bf)

    def desc(t):
        return L.IsaTensor(t.data_ptr(), B, t.shape[1], t.shape[2], t.shape[3], t.shape[3], L.dtype_code(bf), 1)

    def vec(c, lo=0.5):
        return (torch.rand(c, device="cuda", generator=gen) + lo).contiguous()

    def run(fn, reader, what):
        rows = []
        for i in range(REPEATS + 1):
            flush.fill_(i & 1)
            L.check(fn(), what)
            torch.cuda.synchronize()
            L.check(reader(out), "phase trace")
            rows.append(list(out)[:9])
        rows = rows[1:]                                    # the first launch also loads the code object
        med = []
        for k in range(9):
            v = sorted(r[k] - r[0] for r in rows if r[k])
            med.append(v[len(v) // 2] / 100.0 if v else None)
        return med

    print("%-44s %s" % ("launch (32 images, bf16, HBM-cold)", " ".join("%7s" % n for n in NAMES[1:])))
    for N, K, hw in PW:
        g, y, x, dx = tens(hw, N), tens(hw, N, 2.0), tens(hw, K, 2.0), tens(hw, K)
        M = B * hw * hw
        ysc, ysh, ymu, yis = vec(N), vec(N, -0.5), vec(N), vec(N)
        yred = torch.zeros(8 * 2 * N, device="cuda")
        xsc, xsh, xmu, xis = vec(K), vec(K, -0.5), vec(K, 0.0), vec(K)
        xred = torch.zeros(8 * 2 * K, device="cuda")
        W = (torch.randn(N, K, device="cuda", generator=gen) * K ** -0.5).contiguous()
        dw = torch.zeros(N, K, device="cuda")
        ybn = L.IsaBnBwd(L.addr(ysc), L.addr(ysh), L.addr(ymu), L.addr(yis), L.addr(yred), None, None, None, float(M), L.ACT_RELU6)
        xbn = L.IsaBnBwd(L.addr(xsc), L.addr(xsh), L.addr(xmu), L.addr(xis), None, L.addr(xred), None, None, 1.0, 0)
        xpro = L.IsaPro(L.addr(xsc), L.addr(xsh), None, L.ACT_RELU6, None)
        d = [desc(g), desc(y), desc(x), desc(dx)]
        med = run(lambda: lib.isa_conv1x1_bn_backward(C.byref(d[0]), C.byref(d[1]), C.byref(ybn), C.byref(d[2]), C.byref(xpro),
                                                      C.byref(xbn), L.ptr(W), L.ptr(dw), C.byref(d[3]), 0, None, L.ptr(ws),
                                                      ws.numel(), None, st), lib.isa_phase_trace_pw, "pw")
        print("%-44s %s" % ("pw_bn_bwd %d -> %d channels, %dx%d" % (K, N, hw, hw),
                            " ".join("%7s" % ("-" if m is None else "%.2f" % m) for m in med[1:])), flush=True)
    for N, K, hw, form in WG:
        x, dy = tens(hw, K, 2.0), tens(hw, N)
        sc, sh = vec(K), vec(K, -0.5)
        pro = None if form == "none" else L.IsaPro(L.addr(sc), L.addr(sh), None, L.ACT_RELU6, None)
        dw, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
        d = [desc(x), desc(dy)]
        med = run(lambda: lib.isa_conv_wgrad(C.byref(d[0]), C.byref(pro) if pro else None, C.byref(d[1]), L.ptr(dw), L.ptr(db),
                                             L.IN_1X1, L.OUT_PLAIN, None, K, L.ptr(ws), ws.numel(), None, st),
                  lib.isa_phase_trace_wg, "wg")
        print("%-44s %s" % ("conv_wgrad_bf16 %dx%d, %dx%d, %s" % (N, K, hw, hw, form),
                            " ".join("%7s" % ("-" if m is None else "%.2f" % m) for m in med[1:])), flush=True)


if __name__ == "__main__":
    main()
