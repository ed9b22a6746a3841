"""slab_grid (csrc/slab_plan.hpp), the one place that sizes the grid of a weight-gradient launch against its partial-slab
workspace, gives what each of the six launchers it replaced computed for itself.

A small host program (plain C++17, no HIP) includes the header and prints `status gx` over a sweep; the six functions
below restate the launchers as they stood before the header existed, one per site, each taking the site's own `want`
(dwconv.hip launch_wg2: clamp(512 / ncb, 1, ntiles * G); launch_fused: clamp(256 / ncb, 1, ntiles * G);
conv_fused_bwd.hip launch_inst: min((nchunks + 3) / 4 * G, 512); conv_wgrad.hip launch_wg_bf16 / launch_wg:
min((nchunks + 3) / 4 * G, max(512 / (gy * taps), 1)); conv3x3_tiled.hip: min(ntiles, 256)).

Two of the sites do not span the whole sweep, and are compared where they are defined:
  * launch_wg_bf16 / launch_wg kept `want` in two parts, the chunk count w0 and the occupancy cap c; every pair (w0, c) of
    the sweep's values is run through the old code and compared with the plan for min(w0, max(c, 1));
  * conv3x3_wgrad_tiled_launch knew no statistic groups (G = 1) and never clamped from below: for want = 0, which its
    ntiles >= 1 cannot produce, it would have launched an empty grid.  There the plan must give one workgroup.
Every accepted plan is also checked for what makes it safe: G <= gx, gx % G == 0 and gx * set_floats <= ws_floats."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "instance-segmentation-attention_amd", "csrc")

OK, EINVAL, ENOMEM = 0, -1, -5
WANT = [0, 1, 2, 7, 8, 9, 255, 256, 512, 513, 4096]
GROUPS = [1, 2, 3, 8]
SETS = [320, 640, 960, 1056, 2112, 4160, 9504]


def ws_values(st, G):
    return [0, st - 1, st, G * st - 1, G * st, 3 * st, 9 * st, 1 << 24]


PROGRAM = r"""
#include <cstdio>
#include "slab_plan.hpp"
int main() {
    const long wants[] = {%s};
    const int groups[] = {%s};
    const long sets[] = {%s};
    for (long want : wants) for (int G : groups) for (long st : sets) {
        const long wss[] = {0, st - 1, st, G * st - 1, G * st, 3 * st, 9 * st, 1L << 24};
        for (long ws : wss) for (int arena = 0; arena < 2; ++arena) {
            long gx = -1;
            const int rc = slab_grid(want, st, ws, G, arena != 0, &gx);
            std::printf("%%ld %%d %%ld %%ld %%d %%d %%ld\n", want, G, st, ws, arena, rc, rc == ISA_OK ? gx : -1L);
        }
    }
    return 0;
}
""" % tuple(", ".join(str(v) for v in vs) for vs in (WANT, GROUPS, SETS))


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """{(want, G, set_floats, ws_floats, arena): (status, gx)} as the header computes it."""
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = rocm if os.path.isfile(rocm) else shutil.which("c++")
    assert cxx, "no host C++ compiler: neither ROCm's clang++ nor c++"
    d = tmp_path_factory.mktemp("slab_plan")
    src, exe = str(d / "sweep.cpp"), str(d / "sweep")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        want, G, st, ws, arena, rc, gx = (int(v) for v in line.split())
        table[(want, G, st, ws, arena)] = (rc, gx)
    n = sum(2 * len(set(ws_values(st, G))) for _ in WANT for G in GROUPS for st in SETS)     # some workspaces coincide
    assert len(table) == n, (len(table), n)
    return table


def sweep():
    for want, G, st in itertools.product(WANT, GROUPS, SETS):
        for ws, arena in itertools.product(ws_values(st, G), (0, 1)):
            yield want, G, st, ws, arena


# ---- the launchers as they stood, in C's integer arithmetic (every operand is non-negative here) ----------------
def group_grid(gx, G):
    if G <= 1:
        return 1 if gx < 1 else gx
    gx = gx // G * G
    return G if gx < G else gx


def refuse(arena):
    return (ENOMEM if arena else EINVAL), -1


def old_launch_wg2(want, st, ws, G, arena):              # dwconv.hip, st = 10 * 32 * ncb
    gx = want
    ws_cap = ws // st
    if ws_cap < G:
        return refuse(arena)
    if gx > ws_cap:
        gx = ws_cap
    return OK, group_grid(gx, G)


def old_launch_fused(want, st, ws, G, arena):            # dwconv.hip, st = 10 * 32 * ncb
    gx = want
    ws_cap = ws // st
    if ws_cap < G:
        return refuse(arena)
    if gx > ws_cap:
        gx = ws_cap
    gx = group_grid(gx, G)
    return OK, gx


def old_launch_inst(want, st, ws, G, arena):             # conv_fused_bwd.hip, st = TN * TK * 1024 + TN * 32
    gx = want
    ws_cap = ws // st
    if ws_cap < G:
        return refuse(arena)
    if gx > ws_cap:
        gx = ws_cap
    gx = group_grid(gx, G)
    return OK, gx


def old_launch_wg_bf16(w0, c, st, ws, G, arena):         # conv_wgrad.hip, st = slabf * gy * taps, c = 512 / (gy * taps)
    want, cap = w0, c
    ws_cap = ws // st
    if ws_cap < G:
        return refuse(arena)
    if cap > ws_cap:
        cap = ws_cap
    if cap < 1:
        cap = 1
    return OK, group_grid(want if want < cap else cap, G)


def old_launch_wg(w0, c, st, ws, G, arena):              # conv_wgrad.hip, the fp32-MFMA kernel: the same lines
    want, cap = w0, c
    ws_cap = ws // st
    if ws_cap < G:
        return refuse(arena)
    if cap > ws_cap:
        cap = ws_cap
    if cap < 1:
        cap = 1
    gx = group_grid(want if want < cap else cap, G)
    return OK, gx


def old_conv3x3_tiled(want, st, ws, arena):              # conv3x3_tiled.hip, st = 9 * 1056; no groups
    gx = want
    cap = ws // st
    if cap < 1:
        return refuse(arena)
    if gx > cap:
        gx = cap
    return OK, gx


@pytest.mark.parametrize("site", [old_launch_wg2, old_launch_fused, old_launch_inst])
def test_plan_equals_single_want_launchers(plan, site):
    for want, G, st, ws, arena in sweep():
        assert plan[(want, G, st, ws, arena)] == site(want, st, ws, G, arena), (site.__name__, want, G, st, ws, arena)


@pytest.mark.parametrize("site", [old_launch_wg_bf16, old_launch_wg])
def test_plan_equals_fragment_launchers(plan, site):
    for w0, G, st, ws, arena in sweep():
        for c in WANT:
            want = min(w0, max(c, 1))
            assert plan[(want, G, st, ws, arena)] == site(w0, c, st, ws, G, arena), (site.__name__, w0, c, G, st, ws, arena)


def test_plan_equals_conv3x3_tiled_launcher(plan):
    for want, G, st, ws, arena in sweep():
        if G != 1:
            continue
        old = old_conv3x3_tiled(want, st, ws, arena)
        if want == 0 and old[0] == OK:
            assert old[1] == 0                                # the empty grid the old code could not be asked for
            old = (OK, 1)
        assert plan[(want, 1, st, ws, arena)] == old, (want, st, ws, arena)


def test_accepted_plans_fit_the_workspace(plan):
    accepted = 0
    for (want, G, st, ws, arena), (rc, gx) in plan.items():
        if rc != OK:
            assert rc == (ENOMEM if arena else EINVAL) and ws // st < G
            continue
        accepted += 1
        assert gx >= G and gx % G == 0 and gx * st <= ws, (want, G, st, ws, arena, gx)
    assert accepted > len(plan) // 4
