"""Where the label-map operators live: one body each, in isa_amd.labelmaps.LabelOps, reachable through ReSeg and importable
without the model.  No GPU needed."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAUNCH_LEVEL = ("labels_from_planes", "labels_from_onehot", "pair_scores", "sem_scores", "cc_label", "cc_select", "label_props",
                "instance_props", "props_select", "relabel", "contour_trace", "contour_topology", "fill_labels", "cluster",
                "disc_loss", "edt2", "border_map")
PUBLIC = ("score_instances", "semantic_scores", "discriminative_loss", "cluster_embedding", "components", "split_components",
          "clean_instances", "instance_properties", "select_instances", "contour_capacities", "contours", "instance_topology",
          "polygons", "distance_transform", "border_weights", "fill_instances")
# what Network launched for ReSeg before the operators moved; class_map, sem_confusion, onehot_map, argmax_map and
# softmax_nchw read logits of a forward and stay
LEFT_NETWORK = ("distance_transform", "border_weights", "fill_labels", "labels_from_planes", "labels_from_onehot", "disc_loss",
                "cluster", "sem_scores", "cc_label", "cc_select", "label_props", "instance_props", "props_select", "relabel",
                "contour_trace", "contour_topology")


@pytest.mark.parametrize("name", LAUNCH_LEVEL + PUBLIC)
def test_reseg_has_the_operator_and_it_is_the_one_body(name):
    import isa_amd  # noqa: F401
    from isa_amd.labelmaps import LabelOps
    from isa_amd.reseg import ReSeg
    assert issubclass(ReSeg, LabelOps)
    assert callable(getattr(LabelOps, name))
    assert getattr(ReSeg, name) is getattr(LabelOps, name), name


def test_network_keeps_only_what_reads_logits():
    import isa_amd  # noqa: F401
    from isa_amd.network import Network
    assert [name for name in LEFT_NETWORK if hasattr(Network, name)] == []
    for name in ("class_map", "sem_confusion", "onehot_map", "argmax_map", "softmax_nchw"):
        assert callable(getattr(Network, name)), name


def test_no_labelops_attribute_hides_one_of_nn_module():
    import torch.nn as nn
    import isa_amd  # noqa: F401
    from isa_amd.labelmaps import LabelOps
    own = {name for name in vars(LabelOps) if not (name.startswith("__") and name.endswith("__"))} | {"_device", "_alloc", "lib"}
    assert own & set(dir(nn.Module)) == set()


def test_the_module_imports_without_the_model():
    code = ("import sys, isa_amd, isa_amd.labelmaps\n"
            "print(sorted(m for m in ('isa_amd.reseg', 'isa_amd.network', 'isa_amd.model', 'isa_amd.instance_head') "
            "if m in sys.modules))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), check=True,
                         capture_output=True, text=True).stdout
    assert out.strip() == "[]", out


def test_names_that_moved_still_import_from_where_they_were():
    import isa_amd  # noqa: F401
    from isa_amd import labelmaps, network, reseg
    assert network.DiscCriterion is labelmaps.DiscCriterion and network.DISC_FORMS is labelmaps.DISC_FORMS
    assert reseg.PROPS_COLUMNS is labelmaps.PROPS_COLUMNS and len(labelmaps.PROPS_COLUMNS) == 24


def test_a_handle_is_built_without_a_device_and_holds_the_defaults():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    from isa_amd.labelmaps import LabelOps
    ops = LabelOps()
    assert ops.lib is L.checked() and ops.n_classes == 2 and ops._device is None
    assert LabelOps.contour_capacities(256, 256) == (4096, 32768)
    got = []
    LabelOps(alloc=lambda shape, dtype: got.append((shape, dtype))).alloc((3, 4), "dtype")
    assert got == [((3, 4), "dtype")]
