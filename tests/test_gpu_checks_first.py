"""A refused call leaves model state alone.

isa_conv_wgrad, isa_dwconv3x3_wgrad, isa_dwconv3x3_bn_backward, isa_conv1x1_bn_backward and isa_conv_gemm_ep have no
in-kernel form of a pending BatchNorm finalize (isa_pro.fin): they launch isa_bn_finalize themselves, which writes scale /
shift / mean / invstd and updates the running statistics.  They must do so only after every check.  Each case hands an
entry point a real pending finalize whose outputs, and the call's output (dw, or y of the GEMM), hold sentinel values,
makes exactly one argument invalid and requires ISA_EINVAL with every sentinel bit-unchanged.  The invalid argument keeps
every buffer in bounds even if something were launched: a dtype mismatch on a buffer sized for fp32, a workspace whose
stated size is too small while the buffer behind it is large, or an unknown input mode.  The same call with that argument
fixed must succeed and overwrite the sentinels, which shows that the finalize is really pending."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_ops import _gpu  # noqa: E402

ISA_EINVAL = -1
N, H, W, CH = 2, 8, 16, 32                 # every tensor: 2 x 8 x 16 pixels x 32 channels, ld = 32
WS_FLOATS = 1 << 20
STAT_R = 8


def buf(numel, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(numel, generator=g) * scale + offset).cuda()


class Pending:
    """A pending finalize of a CH-channel BatchNorm: its statistics, and its outputs filled with sentinels."""
    OUTS = ("scale", "shift", "mean", "invstd", "running_mean", "running_var")

    def __init__(self, L, act):
        count = float(N * H * W)
        self.stats = buf(STAT_R * 2 * CH, 1, scale=count / STAT_R, offset=1.0)
        self.gamma, self.beta = buf(CH, 2, offset=0.5), buf(CH, 3)
        self.out = {k: torch.full((CH,), 1000.0 + i, device="cuda") for i, k in enumerate(self.OUTS)}
        o = self.out
        self.fin = L.IsaBnFin(self.stats.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(),
                              o["running_mean"].data_ptr(), o["running_var"].data_ptr(), o["scale"].data_ptr(),
                              o["shift"].data_ptr(), o["mean"].data_ptr(), o["invstd"].data_ptr(), count, 0.1, 1e-5, 1)
        self.pro = L.IsaPro(o["scale"].data_ptr(), o["shift"].data_ptr(), None, act, C.pointer(self.fin))


def tensor(L, b, dtype_code):
    """An N x H x W x CH descriptor over `b`, a buffer sized for fp32 whatever the descriptor's dtype."""
    assert b.dtype == torch.float32 and b.numel() == N * H * W * CH
    return L.IsaTensor(b.data_ptr(), N, H, W, CH, CH, dtype_code, 1)


def act_buf(seed, dtype):
    """fp32-sized storage holding an N x H x W x CH tensor of `dtype` at its start."""
    b = torch.zeros(N * H * W * CH, device="cuda")
    v = buf(N * H * W * CH, seed, scale=2.0, offset=-1.0).to(dtype)
    b.view(torch.uint8)[:v.numel() * v.element_size()].copy_(v.view(torch.uint8))
    return b


def bn_bwd(L, keep, act):
    """Backward constants of the BatchNorm after the convolution (read only)."""
    t = [buf(CH, 10, offset=0.5), buf(CH, 11), buf(CH, 12), buf(CH, 13, offset=0.5), buf(STAT_R * 2 * CH, 14)]
    keep.extend(t)
    return L.IsaBnBwd(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                      None, None, None, float(N * H * W), act)


def call(L, lib, entry, pend, out, bad, keep):      # out: the call's output, dw or the GEMM's y
    """Run `entry` with the argument named by `bad` invalid (None: every argument valid)."""
    ws = torch.zeros(WS_FLOATS, device="cuda")
    keep.append(ws)
    ws_floats = 16 if bad == "ws" else WS_FLOATS            # the buffer behind it always holds WS_FLOATS
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pro = C.pointer(pend.pro)
    if entry == "isa_conv_gemm_ep":
        x, w = act_buf(19, torch.float32), buf(CH * CH, 18, offset=-0.5)
        sc, sh = buf(CH, 16, offset=0.5), buf(CH, 17)
        ep = L.IsaConvEp(sc.data_ptr(), sh.data_ptr(), L.ACT_NONE, None)
        keep += [x, w, sc, sh, ep]
        return lib.isa_conv_gemm_ep(tensor(L, x, L.F32), pro, w.data_ptr(), CH, None,
                                    tensor(L, out, L.F32), 3 if bad == "in_mode" else L.IN_1X1,
                                    C.cast(C.pointer(ep), C.c_void_p), st)
    if entry == "isa_conv_wgrad":
        x, dy = act_buf(20, torch.float32), act_buf(21, torch.float32)
        keep += [x, dy]
        return lib.isa_conv_wgrad(tensor(L, x, L.F32), pro, tensor(L, dy, L.BF16 if bad == "dtype" else L.F32),
                                  out.data_ptr(), None, L.IN_1X1, L.OUT_PLAIN, None, 0, ws.data_ptr(), ws_floats, None, st)
    if entry == "isa_dwconv3x3_wgrad":
        x, dy = act_buf(22, torch.float32), act_buf(23, torch.float32)
        keep += [x, dy]
        return lib.isa_dwconv3x3_wgrad(tensor(L, x, L.F32), pro, tensor(L, dy, L.BF16 if bad == "dtype" else L.F32),
                                       out.data_ptr(), None, 0, ws.data_ptr(), ws_floats, None, st)
    ybn = bn_bwd(L, keep, L.ACT_RELU6)
    if entry == "isa_dwconv3x3_bn_backward":
        g, y, x, dx = (act_buf(s, torch.float32) for s in (24, 25, 26, 27))
        w = buf(9 * CH, 28, offset=-0.5)
        keep += [g, y, x, dx, w]
        return lib.isa_dwconv3x3_bn_backward(tensor(L, g, L.F32), tensor(L, y, L.F32), C.pointer(ybn), tensor(L, x, L.F32),
                                             pro, None, w.data_ptr(), out.data_ptr(), 0,
                                             tensor(L, dx, L.BF16 if bad == "dtype" else L.F32), 0, None,
                                             ws.data_ptr(), ws_floats, None, st)
    assert entry == "isa_conv1x1_bn_backward"
    g, y, x, dx = (act_buf(s, torch.bfloat16) for s in (29, 30, 31, 32))
    w = buf(CH * CH, 33, offset=-0.5)
    keep += [g, y, x, dx, w]
    return lib.isa_conv1x1_bn_backward(tensor(L, g, L.BF16), tensor(L, y, L.BF16), C.pointer(ybn), tensor(L, x, L.BF16),
                                       pro, None, w.data_ptr(), out.data_ptr(),
                                       tensor(L, dx, L.F32 if bad == "dtype" else L.BF16), 0, None,
                                       ws.data_ptr(), ws_floats, None, st)


CASES = [(e, bad) for e in ("isa_conv_wgrad", "isa_dwconv3x3_wgrad", "isa_dwconv3x3_bn_backward", "isa_conv1x1_bn_backward")
         for bad in ("dtype", "ws")] + [("isa_conv_gemm_ep", "in_mode")]


@pytest.mark.parametrize("entry,bad", CASES)
def test_refused_call_changes_nothing(entry, bad):
    L, *_ = _gpu()
    lib = L.lib()
    pend = Pending(L, L.ACT_RELU6)
    out = torch.full((N * H * W * CH,), -777.0, device="cuda")  # room for every entry point's dw, and for the GEMM's y
    before = {k: v.clone() for k, v in pend.out.items()}
    out0 = out.clone()
    keep = []
    rc = call(L, lib, entry, pend, out, bad, keep)
    torch.cuda.synchronize()
    assert rc == ISA_EINVAL, (entry, bad, rc)
    for k, v in pend.out.items():
        assert torch.equal(v, before[k]), (entry, bad, k)
    assert torch.equal(out, out0), (entry, bad, "output")
    # the control: the same call, valid, runs the finalize and writes its output
    rc = call(L, lib, entry, pend, out, None, keep)
    torch.cuda.synchronize()
    assert rc == 0, (entry, rc)
    for k, v in pend.out.items():
        assert not torch.equal(v, before[k]), (entry, "finalize did not write", k)
    assert not torch.equal(out, out0), (entry, "output unchanged")
