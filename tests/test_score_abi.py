"""CPU-only: the scoring entry points isa_labels_from_planes / isa_label_pair_hist / isa_instance_scores refuse bad
arguments before they launch anything (so this runs without a GPU: every pointer below is host memory that no kernel may
ever see), and train.py's --val-scores leaves fit's argument tuple alone."""
import os
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
    if name == "isa_labels_from_planes":
        a = dict(planes=buf(), form=L.PLANES_I64_NKHW, n=2, k=4, hw=64, labels=buf(), stream=None)
    elif name == "isa_label_pair_hist":
        a = dict(a=buf(), b=buf(), n=2, L=64, na=5, nb=7, hist=buf(), oob=buf(), mode=L.HIST_AGGREGATE, stream=None)
    else:
        a = dict(hist=buf(), n=2, na=5, nb=7, n_a=buf(), n_b=buf(), out=buf(), stream=None)
    assert len(a) == len(L.SIGNATURES[name]), name
    return a


POINTERS = {"isa_labels_from_planes": ("planes", "labels"), "isa_label_pair_hist": ("a", "b", "hist", "oob"),
            "isa_instance_scores": ("hist", "out")}
BAD_VALUES = {"isa_labels_from_planes": dict(n=(0, -1, 65536), k=(0, -3, 256), hw=(0, -64), form=(-1, 3)),
              "isa_label_pair_hist": dict(n=(0, -1, 65536), na=(0, -1, 257), nb=(0, -1, 257), L=(0, -4, 62, 63, 65),
                                          mode=(-1, 2)),
              "isa_instance_scores": dict(n=(0, -1, 65536), na=(0, -1, 257), nb=(0, -1, 257))}
# the map pointers whose vector loads need alignment
MISALIGNED = {"isa_labels_from_planes": ("planes",), "isa_label_pair_hist": ("a", "b"), "isa_instance_scores": ("hist", "out")}


@pytest.mark.parametrize("name", sorted(POINTERS))
def test_score_entries_refuse_bad_arguments_before_launching(name):
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
    if name != "isa_labels_from_planes":
        for na, nb in ((129, 128), (256, 65), (64, 257)):              # more than 16384 counters
            a = _valid_args(L, name, keep)
            a["na"], a["nb"] = na, nb
            assert fn(*a.values()) == ISA_EINVAL, (name, na, nb)
    for ptr in MISALIGNED[name]:
        a = _valid_args(L, name, keep)
        a[ptr] += 1
        assert fn(*a.values()) == ISA_EALIGN, (name, ptr)


def test_planes_forms_and_alignment():
    """uint8 planes need no alignment; int64 planes 8 bytes, fp32 planes 4."""
    L, lib = _lib()
    keep = []
    for form, off in ((L.PLANES_I64_NKHW, 4), (L.PLANES_F32_NKHW, 2)):
        a = _valid_args(L, "isa_labels_from_planes", keep)
        a["form"] = form
        a["planes"] += off
        assert lib.isa_labels_from_planes(*a.values()) == ISA_EALIGN, (form, off)


def test_val_scores_flag_keeps_the_fit_arguments():
    import train
    plain, on = train.parse_args([]), train.parse_args(['--val-scores'])
    assert plain.val_scores is False and on.val_scores is True
    assert train.fit_arguments(on) == train.fit_arguments(plain)


def test_model_has_the_new_methods():
    import isa_amd  # noqa: F401
    from isa_amd.model import Model
    from isa_amd.reseg import ReSeg
    assert callable(ReSeg.score_instances) and callable(Model.evaluate)
