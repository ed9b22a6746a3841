"""The batched pixel walks of the streaming kernels, at every batch remainder.

bn_bwd_kernel (isa_bn_bwd_reduce / isa_bn_bwd_apply) and materialize_kernel (isa_affine_act_res) issue the loads of U
consecutive trips of their grid-stride walk together (elementwise.hip, STREAM_U_*: U = 2 for bf16; fp32 and the variants
with a per-image multiplier take one trip, all its tensors together).  What a batched loop can get wrong lives at the
batch remainder, so here the number of trips workgroup 0 makes takes every value from 1 to 2U + 1 for each entry point,
always with a ragged last trip (the pixel count is no multiple of a workgroup's pixels per trip, so neither of the
grid's).  Every trip count is asserted from a mirror of the launch code (bn_bwd_grid of test_gpu_streaming.py for the
BatchNorm backward; mat_walk / axpy_walk below).  Per entry point at least one case has a channel tail group (C = 21,
246) and one has bscale / oscale changing between two consecutive trips of a lane (h*w smaller than the grid's pixels
per trip).  isa_axpy's vector kernel, which measured slower when batched and kept its one-item loop, is walked over the
same trip counts (it only takes C % 8 == 0, so it has no tail group).

The checks themselves - the float64 references, the NaN-filled concat buffers whose neighbours must stay bit-unchanged,
and the bounds SUM_BOUND / FP32_BOUND / BF16_STORE - are those of test_gpu_streaming.py, unchanged: each case is run
through that file's test bodies, which print the error per entry point (STREAMERR) before they assert.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_streaming as S  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
U = 2                                   # STREAM_U_REDUCE / _APPLY / _MAT of elementwise.hip (bf16 trips per batch)
TRIPS = list(range(1, 2 * U + 2))       # 1 .. 2U + 1


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ BatchNorm backward
def bn_height(C, apply, k, w, n_per_group=1):
    """Smallest h at which workgroup 0 of the reduce / apply pass makes k trips over n_per_group x h x w pixels, the last
    one ragged."""
    for h in range(1, 40000):
        px = n_per_group * h * w
        if S.bn_bwd_grid(C, px, apply)[2] == k and px % S.bn_ppb(C):
            return h
    raise AssertionError((C, apply, k))


def bn_case(name, which, k, dtype, n, w, C, G, act, bscale, form, h=None):
    if h is None:
        h = bn_height(C, which == "apply", k, w, n // G)
    return (name, dtype, n, h, w, C, G, act, bscale, form, which, k)


# which pass the case aims at, trips of workgroup 0 in it; every case runs both passes.  Narrow path: C = 128 makes k trips
# at about 8192 k px, C = 21 at about 32768 k px, C = 8 at about 131072 k px (k >= 2; one trip needs <= 256 >> sh px).
# Wide path (C > 128, 64 px rows T = cdiv(px, 64)): reduce makes T trips for T <= 4 and cdiv(T, 128) once T > 512; apply
# makes cdiv(T, 512) once T > 1024.  13 images of 3x5 px: bscale changes inside every trip of the grid.
BN_CASES = [
    bn_case("reduce1-w136", "reduce", 1, BF, 1, 5, 136, 1, "relu6", False, "train", h=3),
    bn_case("reduce2-c21-bs", "reduce", 2, BF, 13, 5, 21, 1, "leaky", True, "train", h=3),
    bn_case("reduce3-c128", "reduce", 3, BF, 1, 37, 128, 1, "relu6", False, "chain"),
    bn_case("reduce4-w246-bs", "reduce", 4, F32, 13, 5, 246, 1, "leaky", True, "train", h=3),
    bn_case("reduce5-w136", "reduce", 5, BF, 1, 37, 136, 1, "none", False, "train"),
    bn_case("reduce2-c8-G2", "reduce", 2, F32, 2, 41, 8, 2, "relu", False, "eval"),
    bn_case("reduce4-c128-G2-bs", "reduce", 4, BF, 4, 37, 128, 2, "relu6", True, "chain"),
    bn_case("apply1-c128", "apply", 1, BF, 1, 5, 128, 1, "relu6", False, "chain", h=3),
    bn_case("apply2-w246-eval", "apply", 2, BF, 2, 37, 246, 1, "relu", False, "eval"),
    bn_case("apply3-w136-inplace", "apply", 3, BF, 1, 37, 136, 1, "relu6", False, "chain"),
    bn_case("apply4-c21-train", "apply", 4, BF, 2, 37, 21, 1, "leaky", False, "train"),
    bn_case("apply5-c128-eval", "apply", 5, BF, 1, 37, 128, 1, "relu6", False, "eval"),
    bn_case("apply5-w136-train", "apply", 5, BF, 4, 37, 136, 1, "none", False, "train"),
    bn_case("apply3-c128-f32-bs", "apply", 3, F32, 2, 37, 128, 1, "tanh", True, "train"),
]


def test_bn_cases_cover_every_remainder():
    """Runs without a GPU: the stated trip counts hold for the launch code's grid arithmetic, every trip count 1 .. 2U + 1
    is reached by both passes, and the extra conditions of the module docstring are met."""
    for which in ("reduce", "apply"):
        assert sorted({c[11] for c in BN_CASES if c[10] == which}) == TRIPS, which
    for c in BN_CASES:
        name, _, n, h, w, C, G = c[:7]
        px = n // G * h * w
        grid, _, trips = S.bn_bwd_grid(C, px, c[10] == "apply")
        assert trips == c[11], (name, trips)
        assert px % S.bn_ppb(C) and px % (grid * S.bn_ppb(C)), name          # ragged last trip
    assert any(c[5] % 8 and c[10] == "reduce" for c in BN_CASES)
    assert any(c[5] % 8 and c[10] == "apply" for c in BN_CASES)
    # bscale changes between consecutive trips of a lane: an image is smaller than the grid's pixels per trip
    assert any(c[8] and c[3] * c[4] < S.bn_bwd_grid(c[5], c[2] // c[6] * c[3] * c[4], False)[0] * S.bn_ppb(c[5])
               and c[11] >= 2 for c in BN_CASES)
    forms = {c[9] for c in BN_CASES if c[10] == "apply"}
    assert {"chain", "train", "eval"} <= forms                               # in place, separate dy, eval


@pytest.mark.gpu
@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_bn_bwd_batched(case):
    name, _, n, h, w, C, G = case[:7]
    assert S.bn_bwd_grid(C, n // G * h * w, case[10] == "apply")[2] == case[11]
    S.test_bn_bwd(case[:10])


# ------------------------------------------------------------------------------------------------ isa_affine_act_res
def mat_walk(C, px):
    """isa_affine_act_res: (grid.x, pixels of a workgroup per trip, trips of workgroup 0) per statistic group:
    walk_grid(mkwalk(C, px)) = grid_cap(cdiv(px, 256 >> sh)), cap 2048."""
    cg, sh = cdiv(C, 8), 0
    while (1 << sh) < cg:
        sh += 1
    ppb = 256 >> min(sh, 8)
    grid = min(max(cdiv(px, ppb), 1), 2048)
    return grid, ppb, cdiv(px, grid * ppb)


# name, dtype, n (of x), h, w, C, G, act, parts, fin (as AFF_CASES of test_gpu_streaming.py), trips of workgroup 0.
# k trips need more than 2048 (k - 1) (256 >> sh) px per group: 4096 (k - 1) at C = 1024, 131072 (k - 1) at C = 21.
MAT_CASES = [
    ("mat1-c21", BF, 1, 9, 11, 21, 1, "relu6", "r", None, 1),
    # 17 images of 15x17 = 255 px, 4096 px per trip of the grid: bscale / oscale change inside every trip
    ("mat2-c1024-scales", BF, 17, 15, 17, 1024, 1, "relu6", "r2ob", None, 2),
    ("mat3-c21-oscale", BF, 3, 300, 293, 21, 1, "leaky", "o", None, 3),
    ("mat3-c1024-f32", F32, 33, 15, 17, 1024, 1, "relu6", "2o", None, 3),
    ("mat4-c1024-G2-fin", BF, 2, 111, 113, 1024, 2, "relu6", "r2", 1, 4),
    ("mat5-c1024", BF, 1, 129, 131, 1024, 1, "none", "r", None, 5),
    ("mat5-c24-res2", BF, 2, 511, 517, 24, 1, "relu6", "r2", None, 5),
]


def test_mat_cases_cover_every_remainder():
    assert sorted({c[10] for c in MAT_CASES}) == TRIPS
    for c in MAT_CASES:
        name, _, n, h, w, C, G = c[:7]
        px = n * h * w if "B" in c[8] else n // G * h * w
        grid, ppb, trips = mat_walk(C, px)
        assert trips == c[10], (name, trips)
        assert px % ppb and px % (grid * ppb), name
    assert any(c[5] % 8 for c in MAT_CASES)
    assert any("o" in c[8] and c[3] * c[4] < mat_walk(c[5], c[2] * c[3] * c[4])[0] * mat_walk(c[5], c[2] * c[3] * c[4])[1]
               and c[10] >= 2 for c in MAT_CASES)
    assert any(c[9] is not None and c[6] == 2 for c in MAT_CASES)            # pending finalize with G = 2
    assert any("r" in c[8] for c in MAT_CASES) and any("2" in c[8] for c in MAT_CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MAT_CASES, ids=[c[0] for c in MAT_CASES])
def test_affine_act_res_batched(case):
    S.test_affine_act_res(case[:10])


# ------------------------------------------------------------------------------------------------ isa_axpy
def axpy_walk(C, px):
    """isa_axpy, vector kernel: (grid, trips of workgroup 0): grid_cap(cdiv(px * C / 8, 256)), cap 2048."""
    items = px * (C // 8)
    grid = min(max(cdiv(items, 256), 1), 2048)
    return grid, cdiv(items, grid * 256)


# name, dtype, n, h, w, C, c0 (as AXPY_CASES), trips: k trips need more than 524288 (k - 1) items of 8 channels
AXPY_CASES = [
    ("axpy1", BF, 2, 37, 41, 32, 8, 1), ("axpy2", BF, 8, 97, 101, 64, 8, 2), ("axpy3", F32, 8, 127, 131, 64, 16, 3),
    ("axpy4", BF, 8, 157, 161, 64, 8, 4), ("axpy5", BF, 8, 183, 187, 64, 16, 5),
]


def test_axpy_cases_cover_every_remainder():
    assert sorted({c[7] for c in AXPY_CASES}) == TRIPS
    for name, _, n, h, w, C, c0, k in AXPY_CASES:
        grid, trips = axpy_walk(C, n * h * w)
        assert trips == k, (name, trips)
        assert (n * h * w * (C // 8)) % 256, name                             # ragged last trip


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", AXPY_CASES, ids=[c[0] for c in AXPY_CASES])
def test_axpy_batched(case, accumulate):
    S.test_axpy(case[:7], accumulate, -1.5)
    if case[7] == 3:                     # the fill / no-op form once, on a walk with a full and a remainder batch
        S.test_axpy(case[:7], accumulate, 0.0)
