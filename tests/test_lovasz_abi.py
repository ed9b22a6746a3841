"""CPU-only: isa_segsort_kv_u32 and the isa_lovasz_* entry points refuse bad arguments before they launch anything (so this
runs without a GPU: every pointer below is host memory that no kernel may ever see; the buffers are filled with a sentinel
and must stay as they are), train.py's Lovasz flags parse and leave fit's argument tuple alone, and the Python layers
refuse what they must."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EALIGN, ISA_EDTYPE, ISA_ENOMEM = -1, -2, -3, -5
SENTINEL = 7.25


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


def _tensor(L, data, K=5, n=2, h=4, w=7, ld=8, dtype=None, groups=1, c=None):
    return L.IsaTensor(data, n, h, w, K if c is None else c, ld, L.BF16 if dtype is None else dtype, groups)


def test_signatures_and_tile():
    L, lib = _lib()
    want = dict(isa_segsort_kv_u32=13, isa_lovasz_keys=9, isa_lovasz_coef=9, isa_lovasz_assemble=11, isa_lovasz_grad=7)
    for name, n in want.items():
        assert len(L.SIGNATURES[name]) == n and getattr(lib, name).restype is C.c_int
    hdr = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    assert "#define ISA_SEGSORT_TILE %d\n" % L.SEGSORT_TILE in hdr


def test_segsort_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    b = Bufs(7)
    names = ("keys_in", "vals_in", "keys_out", "vals_out", "nseg", "seglen", "begin", "end", "tmp_keys", "tmp_vals",
             "table", "table_elems", "stream")
    ki, vi, ko, vo, tk, tv, tab = b.ptr
    valid = dict(zip(names, (ki, vi, ko, vo, 3, 100, 0, 32, tk, tv, tab, L.segsort_table_elems(3, 100), None)))
    assert len(valid) == len(L.SIGNATURES["isa_segsort_kv_u32"])
    cases = [(k, None, ISA_EINVAL) for k in ("keys_in", "vals_in", "keys_out", "vals_out", "tmp_keys", "tmp_vals", "table")]
    cases += [("nseg", v, ISA_EINVAL) for v in (0, -1)] + [("seglen", v, ISA_EINVAL) for v in (0, -5, 1 << 31, 1 << 40)]
    cases += [("seglen", (1 << 31) // 3 + 1, ISA_EINVAL)]                 # nseg * seglen >= 2^31
    cases += [("begin", -1, ISA_EINVAL), ("begin", 32, ISA_EINVAL), ("end", 33, ISA_EINVAL), ("end", 0, ISA_EINVAL)]
    # the seven buffers must be distinct: every pair with the same address is refused
    bufs = ("keys_in", "vals_in", "keys_out", "vals_out", "tmp_keys", "tmp_vals", "table")
    cases += [(b1, valid[b0], ISA_EINVAL) for i, b0 in enumerate(bufs) for b1 in bufs[i + 1:]]
    for k in ("keys_in", "vals_in", "keys_out", "vals_out", "tmp_keys", "tmp_vals", "table"):
        cases += [(k, valid[k] + o, ISA_EALIGN) for o in (1, 2)]
    assert L.segsort_table_elems(3, 100) == 3 * 257 and L.segsort_table_elems(2, 9 * L.SEGSORT_TILE) == 2 * (9 * 256 + 2)
    cases += [("table_elems", 3 * 257 - 1, ISA_ENOMEM), ("table_elems", 3 * 256, ISA_ENOMEM), ("table_elems", 0, ISA_ENOMEM)]
    for key, v, want in cases:
        a = dict(valid)
        a[key] = v
        assert lib.isa_segsort_kv_u32(*a.values()) == want, (key, v)
        b.check()
    a = dict(valid, begin=8, end=8)                                       # empty bit range
    assert lib.isa_segsort_kv_u32(*a.values()) == ISA_EINVAL
    a = dict(valid, begin=20, end=12)
    assert lib.isa_segsort_kv_u32(*a.values()) == ISA_EINVAL
    a = dict(valid, seglen=L.SEGSORT_TILE + 1)                            # two tiles need a larger table
    assert lib.isa_segsort_kv_u32(*a.values()) == ISA_ENOMEM
    b.check()


def _bad_logits(L, data):
    """(tensor or None, expected status) for every way the logits can be wrong."""
    yield None, ISA_EINVAL
    yield _tensor(L, None), ISA_EINVAL
    for K in (1, 0, 33):
        yield _tensor(L, data, K=K, ld=40), ISA_EINVAL
    for ld in (12, 20, 4):                                                # ld % 8 != 0, ld < c
        yield _tensor(L, data, ld=ld), ISA_EINVAL
    yield _tensor(L, data, groups=2), ISA_EINVAL
    for n, h, w in ((0, 4, 7), (65536, 4, 7), (2, 0, 7), (2, 4, -1)):
        yield _tensor(L, data, n=n, h=h, w=w), ISA_EINVAL
    yield _tensor(L, data, K=32, ld=32, n=16, h=2048, w=2048), ISA_EINVAL  # K*B*H*W = 2^31
    for dtype in (L.BF16, L.F32):
        for off in (1, 2, 4, 8):
            yield _tensor(L, data + off, dtype=dtype), ISA_EALIGN
    yield _tensor(L, data, dtype=L.F16), ISA_EDTYPE
    yield _tensor(L, data, dtype=7), ISA_EDTYPE


def test_lovasz_keys_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    b = Bufs(5)
    x, lab, keys, vals, G = b.ptr

    def call(t, labels=lab, c0=0, nc=5, per_image=0, keys=keys, vals=vals, G=G):
        rc = lib.isa_lovasz_keys(None if t is None else C.byref(t), labels, c0, nc, per_image, keys, vals, G, None)
        b.check()
        return rc
    for t, want in _bad_logits(L, x):
        assert call(t) == want
    ok = _tensor(L, x)
    for kw in (dict(labels=None), dict(keys=None), dict(vals=None), dict(G=None)):
        assert call(ok, **kw) == ISA_EINVAL, kw
    for c0, nc in ((-1, 2), (0, 0), (0, 6), (4, 2), (5, 1)):              # the class range must lie inside [0, K)
        assert call(ok, c0=c0, nc=nc) == ISA_EINVAL, (c0, nc)
    for kw in (dict(keys=keys + 2), dict(vals=vals + 1), dict(G=G + 2)):
        assert call(ok, **kw) == ISA_EALIGN, kw


def test_lovasz_coef_and_assemble_refuse_bad_arguments_before_launching():
    L, lib = _lib()
    b = Bufs(6)
    k, v, G, tc, part, gp = b.ptr
    names = ("keys", "vals", "G", "nseg", "seglen", "tile_counts", "partial", "gpix", "stream")
    valid = dict(zip(names, (k, v, G, 4, 300, tc, part, gp, None)))
    assert len(valid) == len(L.SIGNATURES["isa_lovasz_coef"])
    cases = [(key, None, ISA_EINVAL) for key in ("keys", "vals", "G", "tile_counts", "partial")]
    cases += [("nseg", 0, ISA_EINVAL), ("nseg", -3, ISA_EINVAL), ("seglen", 0, ISA_EINVAL), ("seglen", 1 << 31, ISA_EINVAL),
              ("seglen", 1 << 29, ISA_EINVAL)]                            # 4 * 2^29 = 2^31
    cases += [(key, valid[key] + 2, ISA_EALIGN) for key in ("keys", "vals", "G", "tile_counts", "gpix")]
    cases += [("partial", part + 4, ISA_EALIGN)]
    for key, val, want in cases:
        a = dict(valid)
        a[key] = val
        assert lib.isa_lovasz_coef(*a.values()) == want, (key, val)
        b.check()
    names = ("partial", "G", "cfg", "B", "K", "per_image", "hw", "segloss", "scale", "scal", "stream")
    valid = dict(zip(names, (part, G, k, 2, 5, 0, 300, tc, v, gp, None)))
    assert len(valid) == len(L.SIGNATURES["isa_lovasz_assemble"])
    cases = [(key, None, ISA_EINVAL) for key in ("partial", "G", "cfg", "segloss", "scale", "scal")]
    cases += [("K", x, ISA_EINVAL) for x in (1, 0, 33)] + [("B", x, ISA_EINVAL) for x in (0, -1)]
    cases += [("hw", 0, ISA_EINVAL), ("hw", -4, ISA_EINVAL), ("hw", 1 << 31, ISA_EINVAL)]
    cases += [("partial", part + 4, ISA_EALIGN), ("segloss", tc + 4, ISA_EALIGN)]
    cases += [(key, valid[key] + 2, ISA_EALIGN) for key in ("G", "cfg", "scale", "scal")]
    for key, val, want in cases:
        a = dict(valid)
        a[key] = val
        assert lib.isa_lovasz_assemble(*a.values()) == want, (key, val)
        b.check()


def test_lovasz_grad_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    b = Bufs(4)
    x, gp, sc, dx = b.ptr

    def call(t, d, gpix=gp, scale=sc):
        rc = lib.isa_lovasz_grad(None if t is None else C.byref(t), gpix, scale, 0, None if d is None else C.byref(d), 0, None)
        b.check()
        return rc
    for t, want in _bad_logits(L, x):
        assert call(t, _tensor(L, dx)) == want
    ok = _tensor(L, x)
    assert call(ok, None) == ISA_EINVAL and call(ok, _tensor(L, None)) == ISA_EINVAL
    assert call(ok, _tensor(L, dx), gpix=None) == ISA_EINVAL and call(ok, _tensor(L, dx), scale=None) == ISA_EINVAL
    for d in (_tensor(L, dx, dtype=L.F32), _tensor(L, dx, n=3), _tensor(L, dx, h=5), _tensor(L, dx, w=8),
              _tensor(L, dx, K=4), _tensor(L, dx, ld=12), _tensor(L, dx, groups=2)):
        assert call(ok, d) == ISA_EINVAL
    assert call(ok, _tensor(L, dx + 8)) == ISA_EALIGN
    assert call(ok, _tensor(L, dx), gpix=gp + 2) == ISA_EALIGN and call(ok, _tensor(L, dx), scale=sc + 1) == ISA_EALIGN


def test_lovasz_flags_keep_the_fit_arguments():
    import train
    plain = train.parse_args([])
    assert plain.lovasz_per_image is False and plain.lovasz_present is False
    for crit in ("Lovasz", "CELovasz"):
        on = train.parse_args(["--criterion", crit, "--lovasz-per-image", "--lovasz-present"])
        assert on.criterion == crit and on.lovasz_per_image is True and on.lovasz_present is True
        a, p = train.fit_arguments(on), train.fit_arguments(plain)
        assert len(a) == len(p) and a[0] == crit and a[1:] == p[1:]
    k = train.parse_args(["--criterion", "CELovasz", "--n-classes", "5", "--semantic-only", "--class-weights", "1,2,3,4,5"])
    assert k.class_weights == [1.0, 2.0, 3.0, 4.0, 5.0]
    with pytest.raises(SystemExit):
        train.parse_args(["--criterion", "Hinge"])


def test_criterion_settings_without_a_device():
    import isa_amd  # noqa: F401
    from isa_amd import network as N
    from isa_amd.model import Model
    assert N.CRITERIA == ("CE", "Dice", "Multi", "Lovasz", "CELovasz")
    crit = N.SemCriterion(3, "cpu")
    assert crit.criterion == "Multi" and not crit.lovasz and crit.cfg.tolist() == [1, 1, 0, 0, 1, 1, 1]
    with pytest.raises(ValueError):
        crit.set("Lovasz", class_weights=[1.0, 2.0, 3.0])
    with pytest.raises(AssertionError):
        crit.set("Hinge")
    crit.set("Lovasz", None, True, lovasz_per_image=True, lovasz_only_present=True)
    assert crit.lovasz and not crit.ce and not crit.dice and not crit.legacy and crit.lovasz_per_image
    assert crit.cfg.tolist() == [0, 0, 1, 1, 1, 1, 1]
    crit.set("CELovasz", [1.0, 2.0, 3.0])
    assert crit.lovasz and crit.ce and not crit.dice and not crit.lovasz_per_image
    assert crit.cfg.tolist() == [1, 0, 0, 0, 1, 2, 3]
    two = N.SemCriterion(2, "cpu")
    assert two.legacy
    two.set("CELovasz")
    assert not two.legacy
    two.set("Multi", lovasz_only_present=True)                             # the flag belongs to the Lovasz criteria alone
    assert two.legacy and two.cfg.tolist() == [1, 1, 0, 0, 1, 1]
    # the scratch of the flagship K = 32, B = 16, 256 x 256 step stays under the budget by sorting classes in groups
    px = 16 * 256 * 256
    kg = N.lovasz_class_group(32, px, True)
    assert 1 <= kg < 32 and 25 * kg * px + 4 * 32 * px <= N.LOVASZ_SCRATCH_BYTES
    assert N.lovasz_class_group(3, 2 * 64 * 64, True) == 3
    import inspect
    sig = inspect.signature(Model.fit).parameters
    assert "lovasz_per_image" in sig and "lovasz_only_present" in sig
