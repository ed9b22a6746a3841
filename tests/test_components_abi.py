"""CPU-only: isa_cc_label / isa_cc_select refuse bad arguments before they launch or clear anything (so this runs without
a GPU: every pointer below is host memory that no kernel may ever see); the host methods exist; the new flags of
pred_list.py / pred.py parse and their defaults leave the existing arguments alone."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EALIGN, ISA_ENOMEM = -1, -2, -5


def _lib():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L, L.lib()


def _valid_args(L, name, keep):
    """A complete, valid argument list of entry `name` over host buffers (64-byte aligned), as a dict in ABI order."""
    buf = lambda: keep.append(torch.zeros(16384)) or keep[-1].data_ptr()            # 64 KiB each
    n, h, w = 2, 8, 12
    if name == "isa_cc_label":
        a = dict(map=buf(), n=n, h=h, w=w, connectivity=8, comp=buf(), n_comp=buf(), scratch=buf(),
                 scratch_bytes=L.cc_label_scratch_bytes(n, h, w), stream=None)
    else:
        a = dict(map=buf(), comp=buf(), n=n, h=h, w=w, mode=L.CC_SPLIT, min_area=1, max_objects=255, out=buf(), count=buf(),
                 dropped=buf(), scratch=buf(), scratch_bytes=L.cc_select_scratch_bytes(n, h, w), stream=None)
    assert len(a) == len(L.SIGNATURES[name]), name
    return a


POINTERS = {"isa_cc_label": ("map", "comp", "n_comp", "scratch"),
            "isa_cc_select": ("map", "comp", "out", "count", "dropped", "scratch")}
SHAPES = dict(n=(0, -1, 65536), h=(0, -8), w=(0, -12, 10, 13, 14))                 # w % 4 != 0 is refused
BAD_VALUES = {"isa_cc_label": dict(SHAPES, connectivity=(0, 1, 6, 9, -4)),
              "isa_cc_select": dict(SHAPES, mode=(-1, 2), max_objects=(0, -1, 256))}
MISALIGNED = {"isa_cc_label": (("map", 1), ("map", 2), ("comp", 4), ("comp", 8), ("n_comp", 2), ("scratch", 8)),
              "isa_cc_select": (("map", 2), ("comp", 4), ("out", 1), ("count", 2), ("dropped", 2), ("scratch", 4))}


@pytest.mark.parametrize("name", sorted(POINTERS))
def test_component_entries_refuse_bad_arguments_before_launching(name):
    L, lib = _lib()
    fn = getattr(lib, name)
    keep = []
    for ptr in POINTERS[name]:
        a = _valid_args(L, name, keep)
        a[ptr] = None
        assert fn(*a.values()) == ISA_EINVAL, (name, ptr)
    for key, values in BAD_VALUES[name].items():
        for v in values:
            a = _valid_args(L, name, keep)
            a[key] = v
            assert fn(*a.values()) == ISA_EINVAL, (name, key, v)
    a = _valid_args(L, name, keep)                                                   # h * w >= 2^30
    a["h"], a["w"] = 1 << 15, 1 << 15
    assert fn(*a.values()) == ISA_EINVAL, (name, "h*w")
    for ptr, off in MISALIGNED[name]:
        a = _valid_args(L, name, keep)
        a[ptr] += off
        assert fn(*a.values()) == ISA_EALIGN, (name, ptr, off)
    a = _valid_args(L, name, keep)
    a["scratch_bytes"] -= 1
    assert fn(*a.values()) == ISA_ENOMEM, name


def test_select_refuses_an_output_that_aliases_the_map():
    L, lib = _lib()
    keep = []
    a = _valid_args(L, "isa_cc_select", keep)
    a["out"] = a["map"]
    assert lib.isa_cc_select(*a.values()) == ISA_EINVAL
    for off in (4, 2 * 8 * 12 - 4):                                                  # overlapping, not equal
        a = _valid_args(L, "isa_cc_select", keep)
        a["out"] = a["map"] + off
        assert lib.isa_cc_select(*a.values()) == ISA_EINVAL, off
    a = _valid_args(L, "isa_cc_select", keep)                                        # right behind the map: no overlap, so the
    a["out"] = a["map"] + 2 * 8 * 12                                                 # next refusal is the scratch size
    a["scratch_bytes"] = 0
    assert lib.isa_cc_select(*a.values()) == ISA_ENOMEM


def test_scratch_formulas_match_the_header():
    L, _ = _lib()
    text = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    assert "#define ISA_CC_TAB_BYTES %d\n" % L.CC_TAB_BYTES in text
    assert "#define ISA_CC_TILE_H %d\n" % L.CC_TILE_H in text and "#define ISA_CC_TILE_W %d\n" % L.CC_TILE_W in text
    assert "enum { ISA_CC_SPLIT = %d, ISA_CC_LARGEST = %d };" % (L.CC_SPLIT, L.CC_LARGEST) in text
    assert L.cc_label_scratch_bytes(3, 8, 12) == 3 * 8 * 12 * 4
    assert L.cc_select_scratch_bytes(3, 8, 12) == 3 * (8 * 12 * 4 + L.CC_TAB_BYTES)


def test_the_new_methods_exist():
    import inspect
    import isa_amd  # noqa: F401
    from isa_amd.model import Model
    from isa_amd.labelmaps import LabelOps
    from isa_amd.reseg import ReSeg
    for cls, names in ((LabelOps, ("cc_label", "cc_select")), (ReSeg, ("components", "split_components", "clean_instances")),
                       (Model, ("predict_components",))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for fn in (Model.predict_instances, Model.evaluate):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("max_objects", "min_area", "keep", "connectivity")] == [None, 0, None, 8]
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("min_area", "keep", "connectivity"))
    p = inspect.signature(ReSeg.clean_instances).parameters
    assert [p[k].default for k in ("keep", "connectivity", "min_area", "max_objects")] == ['largest', 8, 1, 255]


@pytest.mark.parametrize("tool,base", [("pred_list", ["--synthetic", "2"]), ("pred", ["--synthetic"])])
def test_the_new_flags_parse_and_the_defaults_change_nothing(tool, base):
    mod = __import__(tool)
    plain = vars(mod.parse_args(base))
    assert (plain["min_area"], plain["keep"], plain["connectivity"], plain["components"]) == (0, None, 8, False)
    assert mod.cleanup_arguments(mod.parse_args(base)) is None
    # the arguments the tool had before keep their defaults
    assert (plain["instances"], plain["max_objects"], plain["n_classes"], plain["dataset"], plain["model"]) == \
        (False, 32, 2, "CVPPP", "")
    if tool == "pred_list":
        assert (plain["lst"], plain["batch"], plain["synthetic"], plain["output"]) == ("", 16, 2, "")
    on = mod.parse_args(base + ["--instances", "--min-area", "20", "--keep", "largest", "--connectivity", "4"])
    assert mod.cleanup_arguments(on) == {"keep": "largest", "connectivity": 4, "min_area": 20, "max_objects": 32}
    new = {"min_area", "keep", "connectivity", "components", "instances"}
    assert {k: v for k, v in vars(on).items() if k not in new} == {k: v for k, v in plain.items() if k not in new}
    assert mod.cleanup_arguments(mod.parse_args(base + ["--instances", "--min-area", "20"]))["keep"] == "all"
    comp = mod.parse_args(base + ["--components", "--min-area", "9"])
    assert comp.components and comp.min_area == 9 and not comp.instances
    for bad in (["--components", "--instances"], ["--keep", "all"], ["--min-area", "5"], ["--connectivity", "6"],
                ["--instances", "--keep", "some"]):
        with pytest.raises(SystemExit):
            mod.parse_args(base + bad)
