"""CPU-only: train.py's border flags reach Model.fit, pred_list.py's and pred.py's fill flags reach
ReSeg.fill_instances after the clean-up, their defaults change nothing, and a border weight on the Lovasz criterion (which
has no cross-entropy to weigh) is refused."""
import inspect
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def test_border_flags_reach_fit():
    import train
    import isa_amd  # noqa: F401
    from isa_amd.model import Model
    off = train.parse_args([])
    assert (off.border_weight, off.border_sigma) == (0.0, 5.0)
    assert train.fit_keywords(off) == dict(disc_weight=0.0, disc_form='reference', border_weight=0.0, border_sigma=5.0)
    # the positional arguments of fit are the ones the tool passed before
    assert train.fit_arguments(off) == ('Multi', 0.5, 1.5, 2, 1.0, 0.001, 10.0, 0.5, 25, False, 'Adadelta', True, 800, None)
    on = train.parse_args(['--border-weight', '10', '--border-sigma', '3.5', '--disc-weight', '0.25'])
    kw = train.fit_keywords(on)
    assert kw == dict(disc_weight=0.25, disc_form='reference', border_weight=10.0, border_sigma=3.5)
    assert set(kw) <= set(inspect.signature(Model.fit).parameters)
    assert train.fit_arguments(on) == train.fit_arguments(off)
    for bad in (['--border-weight', '-1'], ['--border-sigma', '0'], ['--border-weight', '2', '--criterion', 'Lovasz']):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
    assert train.parse_args(['--border-weight', '2', '--criterion', 'CELovasz']).border_weight == 2.0


class _Net:
    """Stands in for ReSeg: records what the tools ask of it."""

    def __init__(self):
        self.calls = []

    def clean_instances(self, labels, **kw):
        self.calls.append(("clean", labels, kw))
        return "cleaned", "recounted", None

    def class_map(self):
        self.calls.append(("class_map",))
        return "classes"

    def fill_instances(self, labels, fg, **kw):
        self.calls.append(("fill", labels, fg, kw))
        return "filled", None


@pytest.mark.parametrize("tool,base", [("pred_list", ["--synthetic", "2"]), ("pred", ["--synthetic"])])
def test_fill_flags_parse_and_are_passed_on_after_the_clean_up(tool, base):
    mod = __import__(tool)
    import pred_list
    plain = mod.parse_args(base)
    assert (plain.fill, plain.fill_max_dist) == (False, None) and pred_list.fill_arguments(plain) is None
    net = _Net()
    assert pred_list.clean_and_fill(net, "raw", "counts", pred_list.cleanup_arguments(plain),
                                    pred_list.fill_arguments(plain)) == ("raw", "counts")
    assert net.calls == []                                              # with the defaults none of the new code runs
    on = mod.parse_args(base + ["--instances", "--fill"])
    assert pred_list.fill_arguments(on) == {"max_dist": None}
    new = {"fill", "fill_max_dist", "instances"}
    assert {k: v for k, v in vars(on).items() if k not in new} == {k: v for k, v in vars(plain).items() if k not in new}
    both = mod.parse_args(base + ["--instances", "--keep", "largest", "--fill", "--fill-max-dist", "3"])
    assert pred_list.fill_arguments(both) == {"max_dist": 3.0}
    net = _Net()
    got = pred_list.clean_and_fill(net, "raw", "counts", pred_list.cleanup_arguments(both), pred_list.fill_arguments(both))
    assert got == ("filled", "recounted")
    assert [c[0] for c in net.calls] == ["clean", "class_map", "fill"]
    assert net.calls[0][1] == "raw" and net.calls[0][2]["keep"] == "largest"
    assert net.calls[2][1:] == ("cleaned", "classes", {"max_dist": 3.0})    # the cleaned map, the predicted classes
    net = _Net()
    assert pred_list.clean_and_fill(net, "raw", "counts", None, {"max_dist": None}) == ("filled", "counts")
    assert [c[0] for c in net.calls] == ["class_map", "fill"]
    for bad in (["--fill"], ["--instances", "--fill-max-dist", "3"], ["--instances", "--fill", "--fill-max-dist", "-1"],
                ["--components", "--fill"]):
        with pytest.raises(SystemExit):
            mod.parse_args(base + bad)
    if tool == "pred":
        assert inspect.signature(mod.predict_file).parameters["fill"].default is None


def test_lovasz_with_a_border_weight_raises():
    import isa_amd  # noqa: F401
    from isa_amd.network import SemCriterion
    crit = SemCriterion(3, torch.device("cpu"))
    assert not crit.border_on and crit.border_key() is False and crit.border.tolist() == [0.0, 5.0]
    crit.set("Lovasz")
    with pytest.raises(ValueError):
        crit.set_border(10.0)
    assert not crit.border_on
    crit.set("CELovasz")
    crit.set_border(10.0, 4.0)                                         # CELovasz has a CE term to weigh
    assert crit.border_on and crit.border_key() is True and crit.border.tolist() == [10.0, 4.0]
    with pytest.raises(ValueError):
        crit.set("Lovasz")
    for bad in ((-1.0, 5.0), (1.0, 0.0), (1.0, -2.0)):
        with pytest.raises(ValueError):
            crit.set_border(*bad)
    crit.set_border(0.0)
    crit.set("Lovasz")                                                 # off again: fine


def test_the_shipped_combination_leaves_the_legacy_kernels_when_the_border_is_on():
    import isa_amd  # noqa: F401
    from isa_amd.network import SemCriterion
    crit = SemCriterion(2, torch.device("cpu"))
    assert crit.legacy
    ptr = crit.border.data_ptr()
    crit.set_border(10.0)
    assert not crit.legacy and crit.border_on
    crit.set_border_values(2.0, 3.0)                                   # in place: the buffer a captured step reads
    assert crit.border.data_ptr() == ptr and crit.border.tolist() == [2.0, 3.0] and crit.border_on
    crit.set("Multi")
    assert not crit.legacy
    crit.set_border(0.0)
    assert crit.legacy and crit.border.data_ptr() == ptr
