"""CPU-only: the isa_cluster_* entry points exist with the header's signatures and refuse bad arguments before they launch
or write anything (every pointer below is host memory that no kernel may ever see; the buffers are filled with a sentinel and
must stay as they are), the scratch-size macros agree with lib.py, and the Python layers and command lines take the new
options and default to what they did before."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EALIGN, ISA_EDTYPE = -1, -2, -3
SENTINEL = 7.25
NAN, INF = float("nan"), float("inf")


def _lib():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L, L.lib()


class Bufs:
    """Sentinel-filled, 64-byte aligned host buffers; `check` after every refused call."""

    def __init__(self, n):
        self.keep = [torch.full((4096,), SENTINEL) for _ in range(n)]
        self.ptr = [t.data_ptr() for t in self.keep]
        assert all(p % 64 == 0 for p in self.ptr)

    def check(self):
        assert all(bool((b == SENTINEL).all()) for b in self.keep), "a refused call wrote to a buffer"


def _tensor(L, data, c=24, n=2, h=4, w=7, ld=24, dtype=None, groups=1):
    return L.IsaTensor(data, n, h, w, c, ld, L.BF16 if dtype is None else dtype, groups)


def _bad_emb(L, data):
    """(tensor or None, expected status) for every way the embedding can be wrong."""
    yield None, ISA_EINVAL
    yield _tensor(L, None), ISA_EINVAL
    for c, ld in ((0, 8), (33, 40), (40, 40), (-1, 8)):
        yield _tensor(L, data, c=c, ld=ld), ISA_EINVAL
    for ld in (16, 28, 30):                                               # ld < c, ld % 8 != 0
        yield _tensor(L, data, ld=ld), ISA_EINVAL
    yield _tensor(L, data, groups=2), ISA_EINVAL
    for n, h, w in ((0, 4, 7), (65536, 4, 7), (-2, 4, 7), (2, 0, 7), (2, 4, -1), (2, 1 << 16, 1 << 15)):
        yield _tensor(L, data, n=n, h=h, w=w), ISA_EINVAL
    for dtype in (L.BF16, L.F32):
        for off in (1, 2, 4, 8):
            yield _tensor(L, data + off, dtype=dtype), ISA_EALIGN
    yield _tensor(L, data, dtype=L.F16), ISA_EDTYPE
    yield _tensor(L, data, dtype=7), ISA_EDTYPE


def test_signatures_and_size_macros():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    for name, n in dict(isa_cluster_meanshift=15, isa_cluster_kmeans=13).items():
        assert len(L.SIGNATURES[name]) == n and getattr(lib, name).restype is C.c_int
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == n, name
    assert L.SIGNATURES["isa_cluster_meanshift"][2] is C.c_float
    for macro, v in (("ISA_CLUSTER_MAX_SHIFTS", L.CLUSTER_MAX_SHIFTS), ("ISA_CLUSTER_MAX_ITERS", L.CLUSTER_MAX_ITERS),
                     ("ISA_CLUSTER_MAX_ROUNDS", L.CLUSTER_MAX_ROUNDS),
                     ("ISA_CLUSTER_STATE_INTS", L.CLUSTER_STATE_INTS), ("ISA_CLUSTER_CSLAB_STRIDE", L.CLUSTER_CSLAB_STRIDE),
                     ("ISA_DISC_MAX_K", 32)):
        assert "#define %s %d\n" % (macro, v) in hdr
    # ISA_CLUSTER_SCRATCH_BYTES(n, L) = n (8320 + ISA_DISC_CHUNKS(L) 8488): two parities of state (16 ints), centres (32 x 32
    # floats) and, per chunk, a 32 x 32 float slab and ISA_CLUSTER_CSLAB_STRIDE ints; plus two ints per chunk of the init pass
    m = re.search(r"#define ISA_CLUSTER_SCRATCH_BYTES\(n, L\) \(\(int64_t\)\(n\) \* \((\d+) \+ ISA_DISC_CHUNKS\(L\) \* (\d+)\)\)", hdr)
    fixed, per_chunk = int(m.group(1)), int(m.group(2))
    assert fixed == 2 * 4 * (L.CLUSTER_STATE_INTS + 1024) and per_chunk == 2 * 4 * (1024 + L.CLUSTER_CSLAB_STRIDE) + 8
    for n, hw in ((1, 1), (3, 2080), (16, 65536), (2, 1 << 20)):
        assert L.cluster_scratch_bytes(n, hw) == n * (fixed + L.disc_chunks(hw) * per_chunk)
    assert L.cluster_scratch_bytes(16, 65536) == 16 * (8320 + 64 * 8488)


def test_meanshift_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    b = Bufs(8)
    x, fg, lab, nobj, cen, sizes, moved, scratch = b.ptr
    valid = dict(fg=fg, bandwidth=1.5, shifts=3, max_objects=32, max_rounds=32, min_pixels=1, assign_rest=1, labels=lab,
                 n_objects=nobj, centres=cen, sizes=sizes, moved=moved, scratch=scratch)
    assert len(valid) + 2 == len(L.SIGNATURES["isa_cluster_meanshift"])

    def call(t, **kw):
        a = dict(valid)
        a.update(kw)
        rc = lib.isa_cluster_meanshift(None if t is None else C.byref(t), *a.values(), None)
        b.check()
        return rc
    for t, want in _bad_emb(L, x):
        assert call(t) == want
    ok = _tensor(L, x)
    for key in ("fg", "labels", "n_objects", "centres", "sizes", "moved", "scratch"):
        assert call(ok, **{key: None}) == ISA_EINVAL, key
    for kw in (dict(bandwidth=0.0), dict(bandwidth=-1.0), dict(bandwidth=NAN), dict(bandwidth=INF), dict(shifts=-1),
               dict(shifts=9), dict(max_objects=0), dict(max_objects=33), dict(max_objects=-3), dict(min_pixels=0),
               dict(max_rounds=31), dict(max_rounds=0), dict(max_rounds=257), dict(max_objects=4, max_rounds=3),
               dict(min_pixels=-5)):
        assert call(ok, **kw) == ISA_EINVAL, kw
    for kw in (dict(n_objects=nobj + 2), dict(centres=cen + 4), dict(centres=cen + 8), dict(sizes=sizes + 1),
               dict(moved=moved + 2), dict(scratch=scratch + 4), dict(scratch=scratch + 8)):
        assert call(ok, **kw) == ISA_EALIGN, kw


def test_kmeans_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    b = Bufs(10)
    x, fg, nin, init, lab, nobj, cen, sizes, moved, scratch = b.ptr
    valid = dict(fg=fg, n_objects_in=nin, init=init, kmax=32, iters=10, labels=lab, n_objects=nobj, centres=cen, sizes=sizes,
                 moved=moved, scratch=scratch)
    assert len(valid) + 2 == len(L.SIGNATURES["isa_cluster_kmeans"])

    def call(t, **kw):
        a = dict(valid)
        a.update(kw)
        rc = lib.isa_cluster_kmeans(None if t is None else C.byref(t), *a.values(), None)
        b.check()
        return rc
    for t, want in _bad_emb(L, x):
        assert call(t) == want
        assert call(t, init=None) == want
    ok = _tensor(L, x)
    for key in ("fg", "n_objects_in", "labels", "n_objects", "centres", "sizes", "moved", "scratch"):
        assert call(ok, **{key: None}) == ISA_EINVAL, key
    for kw in (dict(kmax=0), dict(kmax=33), dict(kmax=-1), dict(iters=-1), dict(iters=65)):
        assert call(ok, **kw) == ISA_EINVAL, kw
        assert call(ok, init=None, **kw) == ISA_EINVAL, kw
    for kw in (dict(n_objects_in=nin + 2), dict(init=init + 4), dict(init=init + 8), dict(n_objects=nobj + 1),
               dict(centres=cen + 8), dict(sizes=sizes + 2), dict(moved=moved + 1), dict(scratch=scratch + 8)):
        assert call(ok, **kw) == ISA_EALIGN, kw


def test_command_lines_default_to_the_attention_path():
    import pred
    import pred_list
    for mod, base in ((pred_list, ["--synthetic", "4"]), (pred, ["--synthetic"])):
        plain = mod.parse_args(base + ["--instances"])
        assert plain.instances_from == "attention" and plain.bandwidth is None
        assert mod.parse_args(base).instances_from == "attention"
        on = mod.parse_args(base + ["--instances", "--instances-from", "embedding", "--bandwidth", "1.25"])
        assert on.instances_from == "embedding" and on.bandwidth == 1.25
        assert mod.parse_args(base + ["--instances", "--instances-from", "embedding"]).bandwidth is None
        for bad in (["--instances-from", "embedding"], ["--instances", "--bandwidth", "1.0"],
                    ["--instances", "--instances-from", "kmeans"],
                    ["--instances", "--instances-from", "embedding", "--bandwidth", "0"]):
            with pytest.raises(SystemExit):
                mod.parse_args(base + bad)
    sig = inspect.signature(pred.predict_file).parameters
    assert sig["instances_from"].default == "attention" and sig["bandwidth"].default is None


def test_python_layers_take_the_options_without_a_device():
    import isa_amd  # noqa: F401
    from isa_amd.model import Model
    from isa_amd.reseg import ReSeg
    sig = inspect.signature(ReSeg.cluster_embedding).parameters
    assert list(sig)[1:3] == ["emb", "fg"]
    want = dict(method='meanshift', bandwidth=None, delta_var=0.5, delta_dist=1.5, shifts=3, max_objects=32, min_pixels=1,
                assign_rest=True, refine=0, n_objects=None, iters=10, init='farthest', max_rounds=None)
    assert {k: sig[k].default for k in want} == want
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want)
    assert list(inspect.signature(ReSeg.embedding).parameters) == ["self", "x"]
    assert list(inspect.signature(ReSeg.segment_embedding).parameters)[:2] == ["self", "x"]
    for fn in (Model.predict_instances, Model.evaluate):
        sig = inspect.signature(fn).parameters
        assert sig["method"].default == "attention" and sig["bandwidth"].default is None
        assert sig["method"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(Model.predict_instances).parameters["n_objects"].default is None
    # the positional part of the two signatures is what it was
    assert list(inspect.signature(Model.predict_instances).parameters)[:3] == ["self", "images", "max_objects"]
    assert list(inspect.signature(Model.evaluate).parameters)[:3] == ["self", "loader", "max_objects"]
