"""CPU-only checks of the drop-in boundary: the C-ABI library loads and exports every symbol the
header declares; product-side schema equals the oracle's (and the reference's, via the golden run)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]


def test_library_exports_every_declared_symbol():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    declared = set(re.findall(r"\bint\s+(isa_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(L.SIGNATURES), (declared ^ set(L.SIGNATURES))
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    sizes = set(re.findall(r"\bint64_t\s+(isa_[a-z0-9_]+)\s*\(", hdr))         # entry points that return a size
    assert sizes == {"isa_resize_bilinear_ws_bytes"}
    for name in sizes:
        assert hasattr(lib, name), name


def _declarations(ret):
    """{entry point: [parameter text, ...]} of every `<ret> isa_*(...);` in the header, comments stripped."""
    hdr = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    out = {}
    for name, params in re.findall(r"\b%s\s+(isa_[a-z0-9_]+)\s*\(([^()]*)\)\s*;" % ret, hdr):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = [] if params in ([""], ["void"]) else params
    return out


def _assert_matches(L, name, params, argtypes):
    import ctypes as C
    structs = {"isa_tensor": L.P_T, "isa_pro": L.P_PRO, "isa_bn_bwd": L.P_BN}
    scalars = {"int": L.I32, "int32_t": L.I32, "int64_t": L.I64, "float": L.F, "double": L.F64}
    assert len(params) == len(argtypes), "%s: the header declares %d parameters, the binding %d" % (
        name, len(params), len(argtypes))
    for i, (p, t) in enumerate(zip(params, argtypes)):
        where = "%s argument %d (%s)" % (name, i, p)
        words = re.findall(r"\w+", re.sub(r"\bconst\b", " ", p.split("[")[0]))
        base = " ".join(words[:-1])                                  # without the parameter's name
        if "*" in p or "[" in p:
            want = structs.get(base) if p.count("*") == 1 else None
            if want is not None:
                assert t is want, where
            else:                                                    # any other pointer: a pointer slot, never a scalar
                assert issubclass(t, (C.c_void_p, C._Pointer)), where
        else:
            assert base in scalars, where
            assert t is scalars[base], where


def test_signatures_mirror_the_header_argument_by_argument():
    """A wrong width or a missing argument in lib.SIGNATURES would corrupt a call without any error: every declared
    parameter list is compared with the argtypes, position by position."""
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    decl = _declarations("int")
    assert len(decl) >= 112, "only %d declarations parsed" % len(decl)
    assert set(decl) == set(L.SIGNATURES)
    for name, params in decl.items():
        _assert_matches(L, name, params, L.SIGNATURES[name])
    sizes = _declarations("int64_t")
    assert set(sizes) == {"isa_resize_bilinear_ws_bytes"}
    for name, params in sizes.items():
        _assert_matches(L, name, params, getattr(L.lib(), name).argtypes)


def test_pointer_argtype_takes_tensors_and_what_c_void_p_takes():
    import ctypes as C
    import pytest
    import torch
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    memmove = C.CDLL(None)["memmove"]                                # a libc function of its own: (dst, src, n) -> dst
    memmove.argtypes, memmove.restype = [L.VP, L.VP, C.c_size_t], C.c_void_p
    t = torch.arange(16, dtype=torch.int32)
    view = t[5:9]
    assert view.data_ptr() == t.data_ptr() + 20
    for arg, address in ((t, t.data_ptr()), (view, view.data_ptr()), (None, None), (t.data_ptr(), t.data_ptr()),
                         (C.c_void_p(t.data_ptr()), t.data_ptr()), (L.ptr(view), view.data_ptr())):
        assert memmove(arg, arg, 0) == address, arg
    buf = (C.c_int32 * 4)()
    assert memmove(buf, view, 16) == C.addressof(buf) and list(buf) == [5, 6, 7, 8]     # ctypes arrays still pass
    assert memmove(C.byref(buf), t, 16) == C.addressof(buf) and list(buf) == [0, 1, 2, 3]
    with pytest.raises(C.ArgumentError):
        memmove(1.5, t, 0)


def test_raw_handle_returns_the_status_and_checked_handle_raises():
    """One refused call of tests/test_abi_checks_first.py (nothing reaches the GPU) through both handles."""
    import ctypes as C
    import pytest
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    raw, checked = L.lib(), L.checked()
    assert checked is L.checked() and checked.isa_chan_mean is not raw.isa_chan_mean
    for name, argtypes in L.SIGNATURES.items():
        assert list(getattr(checked, name).argtypes) == list(argtypes) == list(getattr(raw, name).argtypes), name
    fin = L.IsaBnFin()
    pro = L.IsaPro(None, None, None, L.ACT_NONE, C.pointer(fin))
    args = [C.pointer(pro) if t is L.P_PRO else None for t in L.SIGNATURES["isa_chan_mean"]]
    assert raw.isa_chan_mean(*args) == -1
    with pytest.raises(L.IsaError, match=r"isa_chan_mean failed: ISA_EINVAL"):
        checked.isa_chan_mean(*args)
    L.check(0, "isa_chan_mean")                                      # a wrapper left around a checked call stays harmless
    need = C.c_int64(-1)                                             # status 0 without a launch: a size query
    assert checked.isa_resize_lanczos_ws_bytes(1, 8, 8, 3, 4, 4, C.byref(need)) == 0 and need.value >= 0
    assert checked.isa_resize_bilinear_ws_bytes(1, 8, 8, 3, 4, 4) == raw.isa_resize_bilinear_ws_bytes(1, 8, 8, 3, 4, 4) >= 0


def test_checked_handle_follows_a_reloaded_library(monkeypatch):
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    before = L.checked()
    monkeypatch.setattr(L, "_lib", None)
    after = L.checked()                                              # built from lib(), which loaded afresh
    assert after is not before and after.raw is L.lib()


def test_missing_library_fails_loudly(monkeypatch):
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    monkeypatch.setattr(L, "LIB_PATH", "/nonexistent/libisa_kernels.so")
    monkeypatch.setattr(L, "_lib", None)
    try:
        L.lib()
    except ImportError as e:
        assert "no CPU fallback" in str(e)
    else:
        raise AssertionError("expected ImportError")


def test_schema_matches_oracle_and_survey_counts():
    import isa_amd  # noqa: F401
    from isa_amd.schema import state_dict_schema as prod
    from reseg_ref import state_dict_schema as orac
    assert prod(True) == orac(True) and prod(False) == orac(False)
    s = prod(True)
    n_el = 0
    for _, shp in s:
        k = 1
        for d in shp:
            k *= d
        n_el += k
    assert len(s) == 891 and n_el == 4824330          # SURVEY.md §8(b) probe of the reference


def test_product_path_never_imports_oracle():
    pkg = os.path.join(ROOT, "instance-segmentation-attention_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            code = "\n".join(l for l in open(os.path.join(pkg, fn)).read().splitlines()
                             if l.lstrip().startswith(("import ", "from ")))
            assert "reseg_ref" not in code and "oracle" not in code and "golden_io" not in code, fn
