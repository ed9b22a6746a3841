"""CPU-only: the isa_disc_* entry points exist with the header's signatures and refuse bad arguments before they launch or
write anything (every pointer below is host memory that no kernel may ever see; the buffers are filled with a sentinel and
must stay as they are), the scratch-size macros agree with lib.py, and the Python layers take the new options."""
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
    want = dict(isa_disc_sums=6, isa_disc_means=11, isa_disc_hinge=10, isa_disc_assemble=15, isa_disc_grad=12)
    hdr = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    for name, n in want.items():
        assert len(L.SIGNATURES[name]) == n and getattr(lib, name).restype is C.c_int
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == n, name
    for macro, v in (("ISA_DISC_MAX_K", L.DISC_MAX_K), ("ISA_DISC_CFG_FLOATS", L.DISC_CFG_FLOATS),
                     ("ISA_DISC_CNT_STRIDE", L.DISC_CNT_STRIDE), ("ISA_ROW_CHUNKS", L.ROW_CHUNKS)):
        assert "#define %s %d\n" % (macro, v) in hdr
    assert [L.disc_chunks(v) for v in (1, 32, 1024, 1025, 2080, 65536, 1 << 20)] == [1, 1, 1, 2, 3, 64, 64]


def test_sums_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    b = Bufs(4)
    x, lab, slab, cslab = b.ptr

    def call(t, labels=lab, k=32, slab=slab, cslab=cslab):
        rc = lib.isa_disc_sums(None if t is None else C.byref(t), labels, k, slab, cslab, None)
        b.check()
        return rc
    for t, want in _bad_emb(L, x):
        assert call(t) == want
    ok = _tensor(L, x)
    for kw in (dict(labels=None), dict(slab=None), dict(cslab=None), dict(k=0), dict(k=33), dict(k=-1)):
        assert call(ok, **kw) == ISA_EINVAL, kw
    for kw in (dict(slab=slab + 4), dict(slab=slab + 8), dict(cslab=cslab + 2)):
        assert call(ok, **kw) == ISA_EALIGN, kw


def _sweep(fn, names, valid, cases, b):
    assert len(valid) == len(names)
    for key, val, want in cases:
        a = dict(zip(names, valid))
        a[key] = val
        assert fn(*a.values()) == want, (key, val)
        b.check()


def test_means_and_assemble_refuse_bad_arguments_before_launching():
    L, lib = _lib()
    b = Bufs(12)
    p = b.ptr
    names = ("slab", "cslab", "n_objects", "cfg", "n", "L", "mu", "m", "mnorm", "cnt", "stream")
    valid = (p[0], p[1], p[2], p[3], 2, 300, p[4], p[5], p[6], p[7], None)
    assert len(names) == len(L.SIGNATURES["isa_disc_means"])
    cases = [(k, None, ISA_EINVAL) for k in ("slab", "cslab", "n_objects", "cfg", "mu", "mnorm", "cnt")]
    cases += [("n", v, ISA_EINVAL) for v in (0, -1, 65536)] + [("L", v, ISA_EINVAL) for v in (0, -4, 1 << 31)]
    cases += [(k, dict(zip(names, valid))[k] + 4, ISA_EALIGN) for k in ("slab", "mu", "m")]
    cases += [(k, dict(zip(names, valid))[k] + 2, ISA_EALIGN) for k in ("cslab", "n_objects", "cfg", "mnorm", "cnt")]
    _sweep(lib.isa_disc_means, names, valid, cases, b)
    names = ("hslab", "partial", "mu", "mnorm", "cnt", "n_objects", "cfg", "norm", "n", "L", "gconst", "coef", "img", "scal",
             "stream")
    valid = (p[0], p[1], p[2], p[3], p[4], p[5], p[6], 2, 2, 300, p[7], p[8], p[9], p[10], None)
    assert len(names) == len(L.SIGNATURES["isa_disc_assemble"])
    ptrs = ("hslab", "partial", "mu", "mnorm", "cnt", "n_objects", "cfg", "gconst", "coef", "img", "scal")
    cases = [(k, None, ISA_EINVAL) for k in ptrs]
    cases += [("norm", v, ISA_EINVAL) for v in (0, 3, -1)] + [("n", v, ISA_EINVAL) for v in (0, -1, 65536)]
    cases += [("L", v, ISA_EINVAL) for v in (0, -4, 1 << 31)]
    cases += [(k, dict(zip(names, valid))[k] + 4, ISA_EALIGN) for k in ("hslab", "mu", "gconst", "partial", "img")]
    cases += [(k, dict(zip(names, valid))[k] + 2, ISA_EALIGN) for k in ("mnorm", "cnt", "n_objects", "cfg", "coef", "scal")]
    _sweep(lib.isa_disc_assemble, names, valid, cases, b)


def test_hinge_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    b = Bufs(7)
    x, lab, nobj, mu, cfg, hslab, part = b.ptr

    def call(t, **kw):
        a = dict(labels=lab, k=32, n_objects=nobj, mu=mu, cfg=cfg, norm=2, hslab=hslab, partial=part)
        a.update(kw)
        rc = lib.isa_disc_hinge(None if t is None else C.byref(t), *a.values(), None)
        b.check()
        return rc
    for t, want in _bad_emb(L, x):
        assert call(t) == want
    ok = _tensor(L, x)
    for key in ("labels", "n_objects", "mu", "cfg", "hslab", "partial"):
        assert call(ok, **{key: None}) == ISA_EINVAL, key
    for kw in (dict(k=0), dict(k=33), dict(norm=0), dict(norm=3), dict(norm=-2)):
        assert call(ok, **kw) == ISA_EINVAL, kw
    for kw in (dict(n_objects=nobj + 2), dict(mu=mu + 4), dict(cfg=cfg + 1), dict(hslab=hslab + 8), dict(partial=part + 4)):
        assert call(ok, **kw) == ISA_EALIGN, kw


def test_grad_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    b = Bufs(8)
    x, lab, nobj, mu, gc, coef, cfg, dx = b.ptr

    def call(t, d, **kw):
        a = dict(labels=lab, k=32, n_objects=nobj, mu=mu, gconst=gc, coef=coef, cfg=cfg, norm=1)
        a.update(kw)
        rc = lib.isa_disc_grad(None if t is None else C.byref(t), *a.values(), None if d is None else C.byref(d), 0, None)
        b.check()
        return rc
    for t, want in _bad_emb(L, x):
        assert call(t, _tensor(L, dx)) == want
    ok = _tensor(L, x)
    assert call(ok, None) == ISA_EINVAL and call(ok, _tensor(L, None)) == ISA_EINVAL
    for key in ("labels", "n_objects", "mu", "gconst", "coef", "cfg"):
        assert call(ok, _tensor(L, dx), **{key: None}) == ISA_EINVAL, key
    for kw in (dict(k=0), dict(k=33), dict(norm=0), dict(norm=3)):
        assert call(ok, _tensor(L, dx), **kw) == ISA_EINVAL, kw
    for d in (_tensor(L, dx, dtype=L.F32), _tensor(L, dx, n=3), _tensor(L, dx, h=5), _tensor(L, dx, w=8),
              _tensor(L, dx, c=16), _tensor(L, dx, ld=28), _tensor(L, dx, groups=2)):
        assert call(ok, d) == ISA_EINVAL
    assert call(ok, _tensor(L, dx + 8)) == ISA_EALIGN
    for kw in (dict(n_objects=nobj + 2), dict(mu=mu + 4), dict(gconst=gc + 8), dict(coef=coef + 1), dict(cfg=cfg + 2)):
        assert call(ok, _tensor(L, dx), **kw) == ISA_EALIGN, kw


def test_disc_flags_keep_the_fit_arguments():
    import train
    plain = train.parse_args([])
    assert plain.disc_weight == 0.0 and plain.delta_var == 0.5 and plain.delta_dist == 1.5 and plain.disc_norm == 2
    assert plain.disc_form == "reference"
    on = train.parse_args(["--disc-weight", "0.25", "--delta-var", "0.75", "--delta-dist", "2.5", "--disc-norm", "1",
                           "--disc-form", "full"])
    a, p = train.fit_arguments(on), train.fit_arguments(plain)
    assert len(a) == len(p)
    diff = [(x, y) for x, y in zip(a, p) if x != y]
    assert diff == [(0.75, 0.5), (2.5, 1.5), (1, 2)]                      # the three values fit() always took
    with pytest.raises(SystemExit):
        train.parse_args(["--disc-norm", "3"])
    with pytest.raises(SystemExit):
        train.parse_args(["--disc-form", "paper"])


def test_python_layers_take_the_options_without_a_device():
    import isa_amd  # noqa: F401
    from isa_amd import network as N
    from isa_amd.model import Model
    from isa_amd.reseg import ReSeg
    from isa_amd.trainer import Trainer
    assert N.DISC_FORMS == {"reference": (True, (1.0, 0.0, 0.0, 0.005)), "full": (False, (1.0, 1.0, 0.001, 0.0))}
    d = N.DiscCriterion("cpu")
    assert not d.on and d.cfg.tolist()[8] == 0.0
    d.set(0.5, delta_var=0.25, delta_dist=2.0, norm=1, form="full")
    assert d.on and d.norm == 1 and d.cfg.tolist() == [0.25, 2.0, 1.0, 0.0, 1.0, 1.0, pytest.approx(0.001), 0.0, 0.5, 0, 0, 0]
    assert d.key() == (True, "full", 1)
    d.set(0.25, form="reference", weights=(1, 2, 3, 4), unit_means=False)
    assert d.cfg.tolist()[3:9] == [0.0, 1.0, 2.0, 3.0, 4.0, 0.25] and d.norm == 2
    for bad in (dict(norm=3), dict(form="paper"), dict(delta_var=-1.0), dict(delta_dist=-0.5), dict(weights=(1, 2, 3))):
        with pytest.raises(ValueError):
            d.set(1.0, **bad)
    with pytest.raises(ValueError):
        d.set(-1.0)
    sig = inspect.signature(Model.fit).parameters
    assert list(sig)[-2:] == ["disc_weight", "disc_form"] and sig["disc_weight"].default == 0.0
    sig = inspect.signature(Trainer.__init__).parameters
    assert [sig[k].default for k in ("disc_weight", "delta_var", "delta_dist", "disc_norm", "disc_form")] == \
        [0.0, 0.5, 1.5, 2, "reference"]
    sig = inspect.signature(ReSeg.discriminative_loss).parameters
    assert list(sig)[1:] == ["emb", "ins", "n_objects", "delta_var", "delta_dist", "norm", "form", "weights", "unit_means",
                             "grad"]
