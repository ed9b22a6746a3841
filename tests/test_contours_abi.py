"""CPU-only: isa_contour_trace / isa_contour_topology refuse bad arguments before they launch anything (so this runs
without a GPU: every pointer below is host memory that no kernel may ever see), the header's constants and scratch
macro equal lib.py's, and the host interface has the new names."""
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EALIGN, ISA_ENOMEM = -1, -2, -5
SIDE = 4096


def _lib():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L, L.lib()


def _valid_args(L, name, keep):
    """A complete, valid argument list of entry `name` over host buffers (64-byte aligned), as a dict in ABI order."""
    buf = lambda: keep.append(torch.zeros(4096)) or keep[-1].data_ptr()
    if name == "isa_contour_trace":
        a = dict(labels=buf(), n=2, h=6, w=8, connectivity=8, cmax=16, vmax=64, table=buf(), verts=buf(), counts=buf(),
                 scratch=buf(), scratch_bytes=L.contour_scratch_bytes(2, 6, 8), stream=None)
    else:
        a = dict(table=buf(), counts=buf(), n=2, cmax=16, nl=16, topo=buf(), stream=None)
    assert len(a) == len(L.SIGNATURES[name]), name
    return a


POINTERS = {"isa_contour_trace": ("labels", "table", "verts", "counts", "scratch"),
            "isa_contour_topology": ("table", "counts", "topo")}
BAD_VALUES = {"isa_contour_trace": dict(n=(0, -1, 65536), h=(0, -6, SIDE + 1), w=(0, -8, SIDE + 4, 6, 7, 9),
                                        connectivity=(0, 6, -8, 1), cmax=(0, -1), vmax=(0, -1)),
              "isa_contour_topology": dict(n=(0, -1, 65536), cmax=(0, -1), nl=(0, -1, 257))}
MISALIGNED = {"isa_contour_trace": (("labels", 1), ("labels", 2), ("table", 4), ("verts", 2), ("counts", 2), ("scratch", 4),
                                    ("scratch", 8)),
              "isa_contour_topology": (("table", 4), ("counts", 2), ("topo", 2))}


@pytest.mark.parametrize("name", sorted(POINTERS))
def test_contour_entries_refuse_bad_arguments_before_launching(name):
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


def test_short_scratch_is_refused_and_the_binding_knows_the_size():
    """One byte less than ISA_CONTOUR_SCRATCH_BYTES is ISA_ENOMEM; exactly that much gets past the size check (and is
    stopped here by a misaligned table, since the size is checked first).  So lib.contour_scratch_bytes is the macro."""
    L, lib = _lib()
    keep = []
    for n, h, w in ((2, 6, 8), (1, 1, 4), (3, 64, 64), (1, 72, 136), (16, 1024, 1024), (1, SIDE, SIDE)):
        a = _valid_args(L, "isa_contour_trace", keep)
        a["n"], a["h"], a["w"] = n, h, w
        a["scratch_bytes"] = L.contour_scratch_bytes(n, h, w) - 1
        assert lib.isa_contour_trace(*a.values()) == ISA_ENOMEM, (n, h, w)
        a["table"] += 4
        assert lib.isa_contour_trace(*a.values()) == ISA_ENOMEM, (n, h, w)
        a["scratch_bytes"] += 1
        assert lib.isa_contour_trace(*a.values()) == ISA_EALIGN, (n, h, w)
    a = _valid_args(L, "isa_contour_trace", keep)
    a["scratch_bytes"] = -1
    assert lib.isa_contour_trace(*a.values()) == ISA_ENOMEM


def test_header_constants_equal_the_binding():
    L, _ = _lib()
    hdr = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert (define("ISA_CONTOUR_MAX_SIDE"), define("ISA_CONTOUR_BLOCK")) == (L.CONTOUR_MAX_SIDE, L.CONTOUR_BLOCK) == (SIDE, 1024)
    assert L.CONTOUR_MAX_SIDE >= 4096
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    import contours_np as C
    assert C.COLS == L.CONTOUR_COLS == 8
    # 48 bytes an edge, 4 a lattice point, 16 per block of either and 16 more, per image
    assert L.contour_scratch_bytes(1, 1, 4) == 16 * 48 + 12 * 4 + 16 + 16 + 16
    assert L.contour_scratch_bytes(3, 64, 64) == 3 * (4 * 4096 * 48 + 4228 * 4 + 5 * 16 + 17 * 16 + 16)


def test_the_host_interface_has_the_new_names():
    import isa_amd  # noqa: F401
    from isa_amd.model import Model
    from isa_amd.labelmaps import LabelOps
    from isa_amd.reseg import ReSeg
    for cls, names in ((LabelOps, ("contour_trace", "contour_topology")),
                       (ReSeg, ("contours", "instance_topology", "polygons")), (Model, ("predict_polygons",))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    p = inspect.signature(ReSeg.contours).parameters
    assert (p["connectivity"].default, p["max_contours"].default, p["max_vertices"].default, p["check"].default) == (
        8, None, None, True)
    p = inspect.signature(ReSeg.instance_topology).parameters
    assert (p["connectivity"].default, p["n_labels"].default) == (8, 256)
    assert inspect.signature(ReSeg.polygons).parameters["connectivity"].default == 8
    assert ReSeg.contour_capacities(256, 256) == (4096, 32768) and ReSeg.contour_capacities(4, 4) == (256, 2048)


def test_polygons_flag_needs_an_instance_source():
    sys.path[:0] = [ROOT]
    import pred_list
    import argparse
    parser = argparse.ArgumentParser()
    pred_list.add_measure_arguments(parser)
    parser.add_argument('--instances', action='store_true')
    parser.add_argument('--components', action='store_true')
    with pytest.raises(SystemExit):
        pred_list.check_measure_arguments(parser, parser.parse_args(['--polygons']))
    for flag in ('--instances', '--components'):
        pred_list.check_measure_arguments(parser, parser.parse_args(['--polygons', flag]))
