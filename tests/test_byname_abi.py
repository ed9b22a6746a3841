"""CPU-only: the seven entry points of the named attention operators (byname_attention.hip) refuse bad arguments before
they launch anything - so this runs without a GPU, and every pointer below is HOST memory that no kernel may ever see:
each call carries exactly one defect (or a defect that is refused ahead of every launch whatever else holds)."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EDTYPE, ISA_ENOMEM = -1, -3, -5
F32, BF16, F16 = 0, 1, 2
NAN, INF = float("nan"), float("inf")
N, H, W = 2, 4, 6


def _lib():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L, L.lib()


class Args:
    """A complete, valid argument list of one entry point over host buffers, as a dict in ABI order; tensors are dicts of
    the isa_tensor fields until the call."""

    def __init__(self, L, name):
        self.L, self.name, self.keep = L, name, []
        buf = lambda: self.keep.append(torch.zeros(16384)) or self.keep[-1].data_ptr()            # 64 KiB each
        ten = lambda c, dtype=F32: dict(data=buf(), n=N, h=H, w=W, c=c, ld=(c + 7) // 8 * 8, dtype=dtype, groups=1)
        if name == "isa_sdp_attention":
            a = dict(q=buf(), k=buf(), v=buf(), mask=buf(), out=buf(), attn=buf(), bh=2, lq=1, L=100, dk=12, dv=12,
                     temperature=12 ** 0.5, dtype=F32, heads=1, mask_per_head=0, ws=buf(), ws_floats=16384, tile_keys=0, stream=None)
        elif name == "isa_sdp_attention_bwd":
            a = dict(q=buf(), k=buf(), v=buf(), attn=buf(), out=buf(), dout=buf(), dq=buf(), dk=buf(), dv=buf(), bh=2, lq=2, L=100,
                     dk_dim=12, dv_dim=12, temperature=12 ** 0.5, dtype=F32, heads=1, stream=None)
        elif name == "isa_sdp_scores":
            a = dict(q=buf(), k=buf(), out=buf(), b=2, heads=1, lq=1, L=100, d=12, dtype=F32, sigmoid=1, stream=None)
        elif name == "isa_linear_ln":
            a = dict(x=buf(), w=buf(), bias=buf(), residual=buf(), gamma=buf(), beta=buf(), eps=1e-5, rows=3, k=24, n=24, y=buf(),
                     stream=None)
        elif name == "isa_instance_norm_res":
            a = dict(x=ten(24), res=ten(24), out=ten(24), eps=1e-5, sums=buf(), stream=None)
        elif name == "isa_local_attention":
            a = dict(q=ten(12), k=ten(12), v=ten(8), nomask=buf(), out=ten(8), dilation=2, scale=0.25, stream=None)
        else:
            a = dict(q=buf(), enc=ten(24), out=buf(), stream=None)
        assert len(a) == len(L.SIGNATURES[name]), name
        self.a = a

    def call(self, lib):
        vals = []
        for v in self.a.values():
            if isinstance(v, dict):
                self.keep.append(self.L.IsaTensor(*v.values()))
                v = C.byref(self.keep[-1])
            vals.append(v)
        return getattr(lib, self.name)(*vals)


def refused(name, rc=ISA_EINVAL, **changes):
    """The entry's valid arguments with `changes` applied (tensor fields as 'tensor.field') are refused with `rc`."""
    L, lib = _lib()
    a = Args(L, name)
    for key, v in changes.items():
        if "." in key:
            t, f = key.split(".")
            assert f in a.a[t], key
            a.a[t][f] = v
        else:
            assert key in a.a, key
            a.a[key] = v
    got = a.call(lib)
    assert got == rc, (name, changes, got)


POINTERS = {
    "isa_sdp_attention": ("q", "k", "v", "out"),                 # mask, attn and ws are optional
    "isa_sdp_attention_bwd": ("q", "k", "v", "attn", "out", "dout", "dq", "dk", "dv"),
    "isa_sdp_scores": ("q", "k", "out"),
    "isa_linear_ln": ("x", "w", "y"),                            # bias, residual, gamma and beta are optional
    "isa_instance_norm_res": ("x", "res", "out", "sums", "x.data", "res.data", "out.data"),
    "isa_local_attention": ("q", "k", "v", "nomask", "out", "q.data", "k.data", "v.data", "out.data"),
    "isa_point_query": ("q", "enc", "out", "enc.data"),
}
# non-positive sizes, sizes over the documented limits, and scalars outside their domain
BAD_VALUES = {
    "isa_sdp_attention": dict(bh=(0, -2), lq=(0, -1), L=(0, -100), dk=(0, -12, 33), dv=(0, -12, 33), heads=(0, -1, 3),
                              temperature=(0.0, -1.0, NAN), tile_keys=(-256, 1, 100, 128, 255, 768, 2048, 4096),
                              ws_floats=(-1,)),
    "isa_sdp_attention_bwd": dict(bh=(0, -2), lq=(0, -1, 9), L=(0, -100), dk_dim=(0, -12, 33, 49), dv_dim=(0, -12, 33, 49),
                                  heads=(0, -1), temperature=(0.0, -1.0, NAN), dtype=(-1, 3, 7)),
    "isa_sdp_scores": dict(b=(0, -2), heads=(0, -1), lq=(0, -1), L=(0, -100), d=(0, -12)),
    "isa_linear_ln": dict(rows=(0, -3), k=(0, -24), n=(0, -24, 65, 1 << 20)),
    "isa_instance_norm_res": {"x.n": (0, -1), "x.h": (0, -1), "x.w": (0, -1), "x.c": (0, -1, 25), "x.ld": (23, 0),
                              "res.n": (0, N + 1), "res.h": (0, H + 1), "res.w": (0, W + 1), "res.c": (0, 16), "res.ld": (23,),
                              "out.n": (0, N + 1, N - 1), "out.h": (0, H + 1, H - 1), "out.w": (0, W + 1, W - 1),
                              "out.c": (0, 16), "out.ld": (23,),
                              "x.dtype": (BF16, F16, -1, 3), "res.dtype": (BF16, F16, 3), "out.dtype": (BF16, F16, 3)},
    "isa_local_attention": {"q.n": (0, N + 1), "q.h": (0, H + 1), "q.w": (0, W + 1), "q.c": (0, 8, 33), "q.ld": (11,),
                            "k.n": (0, N + 1, N - 1), "k.h": (0, H + 1, H - 1), "k.w": (0, W + 1, W - 1), "k.c": (0, 8, 33),
                            "v.n": (0, N + 1, N - 1), "v.h": (0, H + 1, H - 1), "v.w": (0, W + 1, W - 1), "v.c": (0, 12, 33),
                            "out.n": (0, N + 1, N - 1), "out.h": (0, H + 1, H - 1), "out.w": (0, W + 1, W - 1),
                            "out.c": (0, 12, 33), "out.ld": (7,),
                            "q.dtype": (BF16, F16, 3), "k.dtype": (BF16, F16, 3), "v.dtype": (BF16, F16, 3),
                            "out.dtype": (BF16, F16, -1),
                            "dilation": (0, -2), "scale": (0.0, -0.25, NAN, INF, -INF)},
    "isa_point_query": {"enc.n": (0, -1), "enc.h": (0, -1), "enc.w": (0, -1), "enc.c": (0, -1), "enc.ld": (23, 0),
                        "enc.dtype": (F16, -1, 3)},
}


@pytest.mark.parametrize("name", sorted(POINTERS))
def test_entries_refuse_null_pointers_and_bad_sizes_before_launching(name):
    L, _ = _lib()
    assert set(POINTERS) == {k for k in L.SIGNATURES if k.startswith("isa_sdp") or k in (
        "isa_linear_ln", "isa_instance_norm_res", "isa_local_attention", "isa_point_query")}
    for ptr in POINTERS[name]:
        refused(name, **{ptr: None})
    for key, values in BAD_VALUES[name].items():
        for v in values:
            refused(name, **{key: v})


def test_limits_that_take_two_arguments():
    # channel limits of the tensors that travel together: dk / dv 33 and the norm's c 65, every tensor changed alike
    refused("isa_local_attention", **{"q.c": 33, "k.c": 33, "q.ld": 40, "k.ld": 40})
    refused("isa_local_attention", **{"v.c": 33, "out.c": 33, "v.ld": 40, "out.ld": 40})
    refused("isa_instance_norm_res", **{t + f: v for t in ("x", "res", "out") for f, v in ((".c", 65), (".ld", 72))})
    # the backward pass keeps lq * d values of dQ per lane: lq * d <= 96 for d_k and for d_v
    refused("isa_sdp_attention_bwd", lq=8, dk_dim=13)
    refused("isa_sdp_attention_bwd", lq=8, dv_dim=13)
    refused("isa_sdp_attention_bwd", lq=4, dk_dim=25, dv_dim=12)
    # all three storage types agree, bf16 as well as f32 (a uniform bf16 call would be valid: so exactly one differs)
    for odd in ("x", "res", "out"):
        refused("isa_instance_norm_res", **{t + ".dtype": (F32 if t == odd else BF16) for t in ("x", "res", "out")})
    for odd in ("q", "k", "v", "out"):
        refused("isa_local_attention", **{t + ".dtype": (F32 if t == odd else BF16) for t in ("q", "k", "v", "out")})


def test_unknown_dtypes_and_shapes_no_kernel_serves():
    for dt in (-1, 3, 7):
        refused("isa_sdp_attention", ISA_EDTYPE, dtype=dt)
        refused("isa_sdp_scores", ISA_EDTYPE, dtype=dt)
    # interleaved heads and f16 exist at the reference's head width (12) only; d_k != d_v only with one head
    refused("isa_sdp_attention", heads=2, dk=16, dv=16)
    refused("isa_sdp_attention", heads=2, dk=12, dv=8)
    refused("isa_sdp_attention", dtype=F16, dk=16, dv=16)
    refused("isa_sdp_attention", dtype=F16, dk=12, dv=8)
    refused("isa_sdp_attention", heads=2, ws=None)               # without a workspace only the one-head fallback is left
    for tile in (256, 512, 1024):                                # the valid tiles get as far as the next refusal
        refused("isa_sdp_attention", ISA_ENOMEM, tile_keys=tile, ws_floats=0)


def test_sdp_attention_refuses_a_workspace_that_is_too_small():
    # one split of one (head, batch, query) row needs (2 + d) + 2 floats
    for rows, kw in ((1, dict(bh=1)), (2, dict()), (4, dict(heads=2)), (12, dict(heads=2, lq=3))):
        need = rows * (2 + 12) + 2 * rows
        for short in (0, 1, need - 1):
            refused("isa_sdp_attention", ISA_ENOMEM, ws_floats=short, **kw)
