"""CPU-only: train.py's optimizer flags reach Model.fit in the reference's argument order, and the optimizer entry points
isa_adam / isa_rmsprop / isa_sgd refuse bad arguments before they launch anything (so this runs without a GPU: every
pointer below is host memory that no kernel may ever see)."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EALIGN = -1, -2


def test_default_flags_give_the_shipped_fit_arguments():
    import train
    assert train.fit_arguments(train.parse_args([])) == \
        ('Multi', 0.5, 1.5, 2, 1.0, 0.001, 10.0, 0.5, 25, False, 'Adadelta', True, 800, None)


def test_optimizer_flags_land_in_fit_positions():
    import inspect
    import train
    import isa_amd  # noqa: F401
    from isa_amd.model import Model
    args = train.fit_arguments(train.parse_args(['--optimizer', 'SGD', '--lr', '0.01', '--weight-decay', '0', '--freeze-cnn']))
    names = [p for p in inspect.signature(Model.fit).parameters if p != 'self'][:len(args)]
    got = dict(zip(names, args))
    assert got['optimizer'] == 'SGD' and got['learning_rate'] == 0.01 and got['weight_decay'] == 0.0
    assert got['train_cnn'] is False
    assert args == ('Multi', 0.5, 1.5, 2, 0.01, 0.0, 10.0, 0.5, 25, False, 'SGD', False, 800, None)
    for name in ('Adam', 'RMSprop', 'Adadelta'):
        assert train.fit_arguments(train.parse_args(['--optimizer', name]))[10] == name


def test_unknown_optimizer_is_an_argparse_error(capsys):
    import train
    with pytest.raises(SystemExit) as e:
        train.parse_args(['--optimizer', 'Adagrad'])
    assert e.value.code == 2
    assert "--optimizer" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ argument checks
def _valid_args(L, name, keep):
    """A complete, valid argument list of entry `name` over host buffers (64-byte aligned), as a dict in ABI order."""
    buf = lambda: keep.append(torch.zeros(64)) or keep[-1].data_ptr()
    common = dict(sqnorm=buf(), max_norm=1.0, gscale=1.0, lr_dev=None, stream=None)
    if name == "isa_adam":
        a = dict(p=buf(), g=buf(), exp_avg=buf(), exp_avg_sq=buf(), step=buf(), aux=buf(), n=64, lr=1e-3, beta1=0.9,
                 beta2=0.999, eps=1e-8, wd=1e-3)
    elif name == "isa_rmsprop":
        a = dict(p=buf(), g=buf(), square_avg=buf(), n=64, lr=1e-3, alpha=0.99, eps=1e-8, wd=1e-3)
    else:
        a = dict(p=buf(), g=buf(), momentum_buffer=buf(), n=64, lr=1e-2, momentum=0.9, wd=1e-3)
    a.update(common)
    assert len(a) == len(L.SIGNATURES[name]), name
    return a


POINTERS = {"isa_adam": ("p", "g", "exp_avg", "exp_avg_sq", "step", "aux"), "isa_rmsprop": ("p", "g", "square_avg"),
            "isa_sgd": ("p", "g", "momentum_buffer")}
BAD_VALUES = {"isa_adam": dict(lr=(math.nan, math.inf, -1.0), beta1=(1.0, -0.1, math.nan), beta2=(1.0, math.inf),
                               eps=(-1e-8, math.nan), wd=(-1.0, math.inf), gscale=(math.nan,), max_norm=(math.inf,)),
              "isa_rmsprop": dict(lr=(math.nan, -1.0), alpha=(1.5, -0.1, math.nan), eps=(-1.0, math.inf), wd=(math.nan,),
                                  gscale=(math.inf,), max_norm=(math.nan,)),
              "isa_sgd": dict(lr=(math.inf, -1.0), momentum=(-0.5, math.nan, math.inf), wd=(-1e-3,), gscale=(math.nan,),
                              max_norm=(math.nan,))}


@pytest.mark.parametrize("name", sorted(POINTERS))
def test_optimizer_entries_refuse_bad_arguments_before_launching(name):
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    fn = getattr(L.lib(), name)
    keep = []
    for ptr in POINTERS[name]:
        a = _valid_args(L, name, keep)
        a[ptr] = None
        assert fn(*a.values()) == ISA_EINVAL, (name, ptr)
    for n in (0, -5):
        a = _valid_args(L, name, keep)
        a["n"] = n
        assert fn(*a.values()) == ISA_EINVAL, (name, n)
    for key, values in BAD_VALUES[name].items():
        for v in values:
            a = _valid_args(L, name, keep)
            a[key] = v
            assert fn(*a.values()) == ISA_EINVAL, (name, key, v)
    a = _valid_args(L, name, keep)                    # clipping asked for, no norm to read
    a["sqnorm"] = None
    assert fn(*a.values()) == ISA_EINVAL, (name, "sqnorm")
    for ptr in POINTERS[name]:                        # the 16-byte vector accesses need aligned ranges
        if ptr == "step":
            continue
        a = _valid_args(L, name, keep)
        a[ptr] += 4
        assert fn(*a.values()) == ISA_EALIGN, (name, ptr)
