"""CPU-only: isa_sem_confusion / isa_sem_scores refuse bad arguments before they launch or clear anything (so this runs
without a GPU: every pointer below is host memory that no kernel may ever see), train.py's --val-sem-scores leaves fit's
argument tuple alone, and the new methods exist."""
import ctypes as C
import os
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


class Args:
    """A complete, valid argument list of isa_sem_confusion over host buffers (64-byte aligned).  Every buffer is filled
    with a sentinel: an entry that refuses has changed nothing."""

    def __init__(self, L, K=5, n=2, h=4, w=8, ld=8, dtype=None):
        self.L = L
        self.keep = [torch.full((4096,), SENTINEL) for _ in range(5)]
        logits, labels, conf, oob, cmap = [t.data_ptr() for t in self.keep]
        self.t = dict(data=logits, n=n, h=h, w=w, c=K, ld=ld, dtype=L.BF16 if dtype is None else dtype, groups=1)
        self.a = dict(labels=labels, K=K, conf=conf, oob=oob, class_map=cmap)

    def call(self, lib, logits_null=False):
        t = self.L.IsaTensor(self.t["data"], self.t["n"], self.t["h"], self.t["w"], self.t["c"], self.t["ld"],
                             self.t["dtype"], self.t["groups"])
        a = self.a
        rc = lib.isa_sem_confusion(None if logits_null else C.byref(t), a["labels"], a["K"], a["conf"], a["oob"],
                                   a["class_map"], None)
        assert all(bool((b == SENTINEL).all()) for b in self.keep), "a refused call wrote to a buffer"
        return rc


def test_signatures():
    L, lib = _lib()
    assert len(L.SIGNATURES["isa_sem_confusion"]) == 7 and len(L.SIGNATURES["isa_sem_scores"]) == 5
    assert lib.isa_sem_confusion.restype is C.c_int and lib.isa_sem_scores.restype is C.c_int


def test_sem_confusion_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    assert Args(L).call(lib, logits_null=True) == ISA_EINVAL
    a = Args(L); a.t["data"] = None
    assert a.call(lib) == ISA_EINVAL
    # both of labels and class_map NULL; labels given with conf or oob NULL
    a = Args(L); a.a["labels"] = a.a["class_map"] = None
    assert a.call(lib) == ISA_EINVAL
    for ptr in ("conf", "oob"):
        a = Args(L); a.a[ptr] = None
        assert a.call(lib) == ISA_EINVAL, ptr
    for K in (1, 0, -1, 33):
        a = Args(L, K=K); a.t["ld"] = 40
        assert a.call(lib) == ISA_EINVAL, K
    for n in (0, -1, 65536):
        assert Args(L, n=n).call(lib) == ISA_EINVAL, n
    for h, w in ((3, 5), (1, 2), (7, 6)):                             # h*w % 4 != 0
        assert Args(L, h=h, w=w).call(lib) == ISA_EINVAL, (h, w)
    a = Args(L); a.t["c"] = 4                                         # c != K
    assert a.call(lib) == ISA_EINVAL
    for ld in (12, 20, 4):                                            # ld % 8 != 0, ld < c
        assert Args(L, ld=ld).call(lib) == ISA_EINVAL, ld
    a = Args(L); a.t["groups"] = 2
    assert a.call(lib) == ISA_EINVAL
    # alignment: logits 16 bytes, labels and class map 4, conf 8, oob 4
    for dtype in (L.BF16, L.F32):
        for off in (1, 2, 4, 8):
            a = Args(L, dtype=dtype); a.t["data"] += off
            assert a.call(lib) == ISA_EALIGN, (dtype, off)
    for ptr, offs in (("labels", (1, 2)), ("class_map", (1, 2)), ("conf", (1, 4)), ("oob", (1, 2))):
        for off in offs:
            a = Args(L); a.a[ptr] += off
            assert a.call(lib) == ISA_EALIGN, (ptr, off)
    assert Args(L, dtype=L.F16).call(lib) == ISA_EDTYPE
    assert Args(L, dtype=7).call(lib) == ISA_EDTYPE


def test_sem_confusion_null_conf_is_fine_only_without_labels():
    """With labels == NULL, conf and oob may be NULL: the arguments are then valid, so the call is not made here (it would
    launch); with labels given they may not."""
    L, lib = _lib()
    a = Args(L); a.a["conf"] = a.a["oob"] = None
    assert a.call(lib) == ISA_EINVAL


def test_sem_scores_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    conf, out = torch.full((4096,), SENTINEL), torch.full((4096,), SENTINEL)
    valid = dict(conf=conf.data_ptr(), n=2, K=5, out=out.data_ptr(), stream=None)
    assert len(valid) == len(L.SIGNATURES["isa_sem_scores"])
    cases = [("conf", None, ISA_EINVAL), ("out", None, ISA_EINVAL)]
    cases += [("K", v, ISA_EINVAL) for v in (1, 0, -1, 33)] + [("n", v, ISA_EINVAL) for v in (0, -1, 65536)]
    cases += [("conf", valid["conf"] + o, ISA_EALIGN) for o in (1, 4)] + [("out", valid["out"] + o, ISA_EALIGN) for o in (1, 4)]
    for key, v, want in cases:
        a = dict(valid)
        a[key] = v
        assert lib.isa_sem_scores(*a.values()) == want, (key, v)
    assert bool((out == SENTINEL).all())


def test_val_sem_scores_flag_keeps_the_fit_arguments():
    import train
    plain, on = train.parse_args([]), train.parse_args(['--val-sem-scores'])
    assert plain.val_sem_scores is False and on.val_sem_scores is True and on.val_scores is False
    assert train.fit_arguments(on) == train.fit_arguments(plain)
    both = train.parse_args(['--val-sem-scores', '--n-classes', '5', '--semantic-only'])
    assert both.val_sem_scores and both.n_classes == 5


def test_the_new_methods_exist():
    import isa_amd  # noqa: F401
    from isa_amd import parallel
    from isa_amd.model import Model
    from isa_amd.network import Network
    from isa_amd.reseg import ReSeg
    assert callable(Network.class_map) and callable(ReSeg.class_map) and callable(ReSeg.score_semantic)
    assert callable(ReSeg.semantic_scores) and callable(Model.predict_classes) and callable(Model.evaluate_semantic)
    assert callable(parallel.sum_over_ranks)
