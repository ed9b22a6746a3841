"""CPU-only: the float64 restatements of the WHOLE named attention operators (oracle/byname_ref.py) against vectors the
reference's own classes produced off the one configuration of byname_ops.npz (tests/golden/byname_shapes.npz, written by
oracle/gen_golden.py:byname_shape_cases).  Bounds: rtol 1e-5 / atol 1e-6, those of test_oracle_golden.py for the same
operators (the stored vectors are the reference's fp32 results); NaN positions must be the reference's."""
import os

import numpy as np
import pytest
import torch

import byname_ref as B
import golden_io as GIO

RTOL, ATOL = 1e-5, 1e-6


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "byname_shapes.npz"))


def close(got, want, what):
    want = torch.from_numpy(np.asarray(want)).double()
    got = got.double()
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, "NaN positions")
    ok = ~torch.isnan(want)
    err = (got[ok] - want[ok]).abs() - (ATOL + RTOL * want[ok].abs())
    assert float(err.max()) <= 0.0, (what, float(err.max()))


def close_stored(got, z, name):
    """Against a fixture entry: stored in full, or (over STORE_MAX elements) as golden_io's strided sample, compared
    element by element like a full one, plus float64 sums over the whole tensor and its NaN count."""
    if name in z.files:
        return close(got, z[name], name)
    assert tuple(got.shape) == tuple(int(v) for v in z[name + "/shape"]), name
    flat = got.double().reshape(-1)
    assert flat.numel() > B.STORE_MAX
    close(flat[::GIO.subsample_stride(flat.numel(), B.STORE_MAX)], z[name + "/sub"], name + "/sub")
    s, sabs, ssq, nans = (float(v) for v in z[name + "/sums"])
    ok = flat[~torch.isnan(flat)]
    assert int(torch.isnan(flat).sum()) == int(nans), name
    assert abs(float(ok.abs().sum()) - sabs) <= RTOL * sabs and abs(float((ok * ok).sum()) - ssq) <= 2 * RTOL * ssq, name
    assert abs(float(ok.sum()) - s) <= RTOL * sabs, name


def sd_of(z, pre):
    return {k[len(pre) + 3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre + "sd/")}


def stored_or_drawn(z, pre, names, drawn):
    """The case's inputs: the stored arrays, which must be what the seed draws; the ones too large to store from the seed."""
    out = []
    for nm, t in zip(names, drawn):
        if pre + nm in z.files:
            assert np.array_equal(z[pre + nm], t.numpy()), (pre, nm)
        else:
            assert t.numel() > B.STORE_MAX, (pre, nm)
        out.append(t)
    return out


def spd_case(z, i):
    pre = "spd%d/" % i
    assert tuple(int(v) for v in z[pre + "case"]) == B.SPD_CASES[i]
    qk, v, nomask = stored_or_drawn(z, pre, ("qk_in", "v_in", "nomask"), B.spd_inputs(i))
    return pre, sd_of(z, pre), qk, v, nomask


def mha_case(z, i):
    pre = "mha%d/" % i
    assert tuple(int(v) for v in z[pre + "case"]) == B.MHA_CASES[i]
    q, k, v, mask = B.mha_inputs(i)
    q, k, v = stored_or_drawn(z, pre, ("q", "k", "v"), (q, k, v))
    assert np.array_equal(z[pre + "mask_bits"], np.packbits(mask.numpy().reshape(-1)))
    return pre, sd_of(z, pre), q, k, v, mask


def test_fixture_is_data_of_the_listed_cases_and_small(z, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "byname_shapes.npz")) < 1 << 20
    pres = sorted(set(k.split("/")[0] for k in z.files))
    assert pres == sorted(["spd%d" % i for i in range(len(B.SPD_CASES))] + ["mha%d" % i for i in range(len(B.MHA_CASES))] +
                          ["dec%d" % i for i in range(len(B.DEC_CASES))])
    assert all(z[k].dtype.kind in "fiub" for k in z.files)           # numbers only
    # the coincidence of byname_ops.npz (c == d_k) must not be the rule here, and the perturbed affine terms are there
    assert sum(dm // G != dk for dk, dv, dm, G, *_ in B.SPD_CASES) >= 3
    assert float(np.abs(z["mha0/sd/layer_norm.bias"]).min()) > 0 and float(np.abs(z["mha0/sd/layer_norm.weight"] - 1).min()) > 0
    assert float(np.abs(z["spd0/sd/fc.bias"]).max()) > 0.05


@pytest.mark.parametrize("i", range(len(B.SPD_CASES)))
def test_scale_pd_attention_restatement(z, i):
    pre, sd, qk, v, nomask = spd_case(z, i)
    dil = B.SPD_CASES[i][4]
    taps = {}
    out = B.scale_pd_attention(sd, qk, v, nomask, dil, taps=taps)
    assert out.dtype == torch.float64
    for nm in ("QK", "V", "att"):
        close_stored(taps[nm], z, pre + nm)
    close_stored(out, z, pre + "out")


@pytest.mark.parametrize("i", [i for i, (dk, dv, dm, G, *_) in enumerate(B.SPD_CASES) if dm // G != dk])
def test_dk_scale_misses_the_reference_off_the_coincidence(z, i):
    """Guard of the fixture: with d_k ** -0.5 in place of the reference's c ** -0.5 the attended map is off by more than
    1e-2 of its largest element wherever c != d_k, so these cases can tell the two apart."""
    pre, sd, qk, v, nomask = spd_case(z, i)
    dk, dv, dm, G, dil = B.SPD_CASES[i][:5]
    taps = {}
    B.scale_pd_attention(sd, qk, v, nomask, dil, scale=dk ** -0.5, taps=taps)
    got = taps["att"]
    if pre + "att" in z.files:
        want = torch.from_numpy(z[pre + "att"]).double()
    else:
        want = torch.from_numpy(z[pre + "att/sub"]).double()
        got = got.reshape(-1)[::GIO.subsample_stride(got.numel(), B.STORE_MAX)]
    miss = float((got - want).abs().max() / want.abs().max())
    assert miss > 1e-2, (B.SPD_CASES[i], miss)


@pytest.mark.parametrize("i", range(len(B.MHA_CASES)))
def test_multi_head_attention_restatement(z, i):
    pre, sd, q, k, v, mask = mha_case(z, i)
    G, dm, dk, dv, b, lq, L = B.MHA_CASES[i]
    out, attn = B.multi_head_attention(sd, G, dk, dv, q, k, v, mask)
    assert out.dtype == torch.float64
    close_stored(out, z, pre + "out")
    close_stored(attn, z, pre + "attn")
    last, none = B.multi_head_attention(sd, G, dk, dv, q, k, v, mask, last=True)
    assert none is None
    close_stored(last, z, pre + "last")
    nan_rows = torch.isnan(out).all(2)
    if i == 0:        # the planted row: NaN in every element of its output row and in its attention row of either head
        want = torch.zeros(b, lq, dtype=torch.bool)
        want[B.MHA_MASKED_ROW] = True
        assert torch.equal(nan_rows, want) and torch.equal(torch.isnan(out).any(2), want)
        assert torch.equal(torch.isnan(attn).all(2), want.repeat(G, 1))
        assert not torch.isnan(last).any()            # the last=True branch reads no mask
    else:
        assert not nan_rows.any() and not torch.isnan(attn).any()


@pytest.mark.parametrize("i", range(len(B.DEC_CASES)))
def test_point_query_restatement(z, i):
    pre = "dec%d/" % i
    assert tuple(int(v) for v in z[pre + "case"]) == B.DEC_CASES[i]
    q, enc = stored_or_drawn(z, pre, ("q", "enc"), B.dec_inputs(i))
    close_stored(B.point_query_mask(q, enc), z, pre + "out")


def test_core_restatements_in_float64_on_the_old_fixture(golden_dir):
    """The sdp core and the default scale (None = d_k ** -0.5) on byname_ops.npz, evaluated in float64."""
    import reseg_ref as R
    z0 = np.load(os.path.join(golden_dir, "byname_ops.npz"))
    t = lambda k: torch.from_numpy(z0[k])
    out, attn = B.sdp_attention(t("sdp/q"), t("sdp/k"), t("sdp/v"), 12 ** 0.5, t("sdp/mask"))
    close(out, z0["sdp/out"], "sdp/out")
    close(attn, z0["sdp/attn"], "sdp/attn")
    QK, V = t("local/QK").double(), t("local/V").double()
    nm = t("local/nomask").double().repeat(2, 1, 1, 1)
    a = R.local_dilated_attention(QK[:, :12], QK[:, 12:], V, nm, 2)
    b = R.local_dilated_attention(QK[:, :12], QK[:, 12:], V, nm, 2, scale=12 ** -0.5)
    assert torch.equal(a, b)
    close(a.contiguous().view(2, 24, 16, 16), z0["local/att"], "local/att")
    sd = {k[len("local/sd/"):]: t(k) for k in z0.files if k.startswith("local/sd/")}
    close(B.scale_pd_attention(sd, t("local/qk_in"), t("local/v_in"), t("local/nomask"), 2), z0["local/out"], "local/out")
    sd = {k[len("mha/sd/"):]: t(k) for k in z0.files if k.startswith("mha/sd/")}
    o, a = B.multi_head_attention(sd, 2, 12, 12, t("mha/q"), t("mha/k"), t("mha/v"), t("mha/mask"))
    close(o, z0["mha/out"], "mha/out")
    close(a, z0["mha/attn"], "mha/attn")
