"""CPU-only: the measuring entry points isa_label_props / isa_instance_props / isa_props_select / isa_relabel_u8 refuse bad
arguments before they launch anything (so this runs without a GPU: every pointer below is host memory that no kernel may
ever see), the header's constants equal lib.py's, and the host interface has the new names."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EALIGN = -1, -2


def _lib():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L, L.lib()


def _valid_args(L, name, keep):
    """A complete, valid argument list of entry `name` over host buffers (64-byte aligned), as a dict in ABI order."""
    buf = lambda: keep.append(torch.zeros(4096)) or keep[-1].data_ptr()
    if name == "isa_label_props":
        a = dict(labels=buf(), image=buf(), n=2, h=6, w=6, c=4, nl=16, acc=buf(), oob=buf(), stream=None)   # 7 * 6 % 4 != 0
    elif name == "isa_instance_props":
        a = dict(acc=buf(), n=2, nl=16, h=8, w=8, c=3, out=buf(), stream=None)
    elif name == "isa_props_select":
        a = dict(acc=buf(), n=2, nl=16, h=8, w=8, min_area=1, max_area=0, clear_border=0, order=L.ORDER_AREA, max_objects=255,
                 table=buf(), count=buf(), dropped=buf(), stream=None)
    else:
        a = dict(labels=buf(), table=buf(), n=2, L=64, out=buf(), stream=None)
    assert len(a) == len(L.SIGNATURES[name]), name
    return a


SIDE = 32768
POINTERS = {"isa_label_props": ("labels", "image", "acc", "oob"), "isa_instance_props": ("acc", "out"),
            "isa_props_select": ("acc", "table", "count", "dropped"), "isa_relabel_u8": ("labels", "table", "out")}
BAD_VALUES = {"isa_label_props": dict(n=(0, -1, 65536), h=(0, -8, SIDE + 1, 7), w=(0, -8, SIDE + 1, 7), c=(-1, 2, 5, 0),
                                      nl=(0, -1, 257)),
              "isa_instance_props": dict(n=(0, -1, 65536), h=(0, -8, SIDE + 1), w=(0, -8, SIDE + 1), c=(-1, 2, 5),
                                         nl=(0, -1, 257)),
              "isa_props_select": dict(n=(0, -1, 65536), h=(0, -8, SIDE + 1), w=(0, -8, SIDE + 1), nl=(0, -1, 257),
                                       min_area=(-1,), max_area=(-1,), clear_border=(-1, 2), order=(-1, 3),
                                       max_objects=(0, -1, 256)),
              "isa_relabel_u8": dict(n=(0, -1, 65536), L=(0, -4, 62, 63, 65, 1 << 31))}
MISALIGNED = {"isa_label_props": (("labels", 1), ("labels", 2), ("image", 1), ("acc", 4), ("oob", 2)),
              "isa_instance_props": (("acc", 4), ("out", 4)),
              "isa_props_select": (("acc", 4), ("count", 2), ("dropped", 2)),
              "isa_relabel_u8": (("labels", 1), ("out", 2))}


@pytest.mark.parametrize("name", sorted(POINTERS))
def test_props_entries_refuse_bad_arguments_before_launching(name):
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
    for ptr, off in MISALIGNED[name]:
        a = _valid_args(L, name, keep)
        a[ptr] += off
        assert fn(*a.values()) == ISA_EALIGN, (name, ptr, off)


def test_image_and_channels_go_together():
    """c == 0 means no image and an image means c in {1, 3, 4}; only c == 4 asks for an aligned image."""
    L, lib = _lib()
    keep = []
    a = _valid_args(L, "isa_label_props", keep)
    a["c"], a["image"] = 0, None
    b = _valid_args(L, "isa_label_props", keep)
    b["c"], b["image"] = 0, b["labels"]
    assert lib.isa_label_props(*b.values()) == ISA_EINVAL
    for c in (1, 3):
        d = _valid_args(L, "isa_label_props", keep)
        d["c"] = c
        d["acc"] += 4                                                    # stops every call here at the alignment check
        d["image"] += 1
        assert lib.isa_label_props(*d.values()) == ISA_EALIGN
    a["acc"] += 4
    assert lib.isa_label_props(*a.values()) == ISA_EALIGN                # c == 0 with NULL got past the argument check


def test_relabel_refuses_partial_overlap():
    L, lib = _lib()
    keep = []
    a = _valid_args(L, "isa_relabel_u8", keep)
    a["out"] = a["labels"] + 64                                          # 2 * 64 bytes each: the second half overlaps
    assert lib.isa_relabel_u8(*a.values()) == ISA_EINVAL
    a["out"] = a["labels"] - 64
    assert lib.isa_relabel_u8(*a.values()) == ISA_EINVAL


def test_header_constants_equal_the_binding():
    L, _ = _lib()
    hdr = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert (define("ISA_PROPS_ACC"), define("ISA_PROPS_OUT"), define("ISA_PROPS_MAX_SIDE")) == (
        L.PROPS_ACC, L.PROPS_OUT, L.PROPS_MAX_SIDE) == (16, 24, SIDE)
    m = re.search(r"enum\s*\{\s*ISA_ORDER_LABEL\s*=\s*(\d+),\s*ISA_ORDER_AREA\s*=\s*(\d+),\s*ISA_ORDER_RASTER\s*=\s*(\d+)", hdr)
    assert tuple(int(t) for t in m.groups()) == (L.ORDER_LABEL, L.ORDER_AREA, L.ORDER_RASTER)
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    import props_np as P
    assert (P.ACC, P.OUT, P.ORDER_LABEL, P.ORDER_AREA, P.ORDER_RASTER) == (L.PROPS_ACC, L.PROPS_OUT, L.ORDER_LABEL,
                                                                            L.ORDER_AREA, L.ORDER_RASTER)
    from isa_amd import reseg
    assert reseg.PROPS_COLUMNS == P.COLUMNS and len(reseg.PROPS_COLUMNS) == L.PROPS_OUT


def test_the_host_interface_has_the_new_names():
    import inspect
    import isa_amd  # noqa: F401
    from isa_amd.model import Model
    from isa_amd.labelmaps import LabelOps
    from isa_amd.reseg import ReSeg
    for cls, names in ((LabelOps, ("label_props", "props_select", "relabel")),
                       (ReSeg, ("instance_properties", "select_instances")), (Model, ("measure_instances",))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for fn in (Model.predict_instances, Model.evaluate):
        p = inspect.signature(fn).parameters
        assert (p["order"].default, p["clear_border"].default, p["max_area"].default) == (None, False, None)
    p = inspect.signature(ReSeg.select_instances).parameters
    assert (p["min_area"].default, p["max_area"].default, p["clear_border"].default, p["order"].default,
            p["max_objects"].default) == (1, None, False, 'label', 255)
