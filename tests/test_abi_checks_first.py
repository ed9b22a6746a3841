"""CPU-only: entry points that take an isa_pro check their arguments before they touch them.

Every call below passes x = NULL and a pro whose fin (a pending BatchNorm finalize) is non-NULL with all-NULL fields.
Every tensor and buffer pointer is NULL; only the descriptor structs live in host memory, as the ABI requires.  An entry
point that read x->c, or launched the finalize, before its checks would dereference NULL on the host; a correct one
returns ISA_EINVAL without reaching the GPU, so this runs on a machine without one."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL = -1
ENTRY_POINTS = ["isa_conv_gemm", "isa_conv_gemm_ep", "isa_conv_wgrad", "isa_dwconv3x3", "isa_dwconv3x3_wgrad",
                "isa_dwconv3x3_bn_backward", "isa_conv1x1_bn_backward", "isa_affine_act_res", "isa_chan_mean"]


def test_null_input_with_pending_finalize_is_refused():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    lib = L.lib()
    fin = L.IsaBnFin()                                   # every field NULL / 0
    pro = L.IsaPro(None, None, None, L.ACT_NONE, C.pointer(fin))
    ep = L.IsaConvEp()                                   # isa_conv_gemm_ep refuses a NULL ep before anything else
    for name in ENTRY_POINTS:
        sig = L.SIGNATURES[name]
        assert sig.count(L.P_PRO) == 1, name
        args = []
        for t in sig:
            if t is L.P_PRO:
                args.append(C.pointer(pro))
            elif t in (L.I32, L.I64):
                args.append(0)
            else:
                args.append(None)                        # tensors, buffers, streams, BN descriptors: NULL
        if name == "isa_conv_gemm_ep":
            args[7] = C.cast(C.pointer(ep), C.c_void_p)
        assert getattr(lib, name)(*args) == ISA_EINVAL, name
