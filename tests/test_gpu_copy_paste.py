"""isa_copy_paste_u8 against tests/copy_paste_np.py, bit for bit, through the C-ABI.  On every shape: the cases of
tests/test_copy_paste_ref.py built programmatically (no flip or shift, each flip, a shift that cuts at the border, full
occlusion, capacity, min_area, garbage behind the counts, s == b, s outside the batch) and random transforms with shifts
up to the full side.  The sub-cases the kernels branch on are asserted to occur, on the restatement's plan, before anything
is compared.  Outputs and scratch are poisoned before every call."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import copy_paste_np as CP   # noqa: E402

# (n, h, w, k, c): odd sides, tail lanes and the vector path; one 16-byte vector; the scalar path with c = 1; several
# workgroups per image (the counters across workgroups, "the first workgroup writes the plan")
SHAPES = [(3, 37, 53, 32, 3), (2, 16, 16, 16, 3), (4, 9, 130, 6, 1), (2, 70, 300, 32, 4)]


def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L, L.lib()


def popcount(v):
    return bin(int(v)).count("1")


def scene(shape, seed=0):
    """A batch in which every plane of every image holds an instance (so whatever lies behind a count is garbage): random
    rectangles with byte values 1, 7 and 255, except that plane 0 of image 0 is a 2 x 2 square which plane 0 of image 1
    covers, and plane 1 of image 1 has two pixels in the last row."""
    n, h, w, k, c = shape
    rng = np.random.default_rng(100 + seed)
    planes = np.zeros((n, h, w, k), np.uint8)
    for b in range(n):
        for i in range(k):
            y0, x0 = rng.integers(0, h - 2), rng.integers(0, w - 2)
            planes[b, y0:y0 + rng.integers(2, h // 2), x0:x0 + rng.integers(2, w // 2), i] = (1, 7, 255)[rng.integers(3)]
    planes[0, :, :, 0] = 0
    planes[0, 1:3, 1:3, 0] = 1
    planes[1, :, :, 0] = 0
    planes[1, :h // 2, :w // 2, 0] = 7
    planes[1, :, :, 1] = 0
    planes[1, h - 1, w - 2:, 1] = 255
    rgb = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    sem = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    return rgb, sem, planes


def cases(shape):
    """(name, counts, xform, select, min_area) over scene(shape)."""
    n, h, w, k, c = shape
    rng = np.random.default_rng(7)
    ring = [((b + 1) % n, 0, 0, 0) for b in range(n)]
    half, ones = [k // 2] * n, [0xffffffff] * n
    out = [("plain", half, ring, ones, 1)]
    out.append(("flips", half, [((b + 1) % n, 1 + b % 3, 0, 0) for b in range(n)], ones, 1))
    out.append(("flip_y", half, [((b + 1) % n, 2, 0, 0) for b in range(n)], ones, 1))
    out.append(("both_flips", half, [((b + 1) % n, 3, 1, -1) for b in range(n)], ones, 1))
    out.append(("border", half, [((b + 1) % n, 0, (-1) ** b * (h // 3), -(-1) ** b * (w // 3)) for b in range(n)], ones, 1))
    out.append(("occlusion", [2] + [k] * (n - 1), [(1, 0, 0, 0)] + [(-1, 0, 0, 0)] * (n - 1), [0b1] * n, 1))
    out.append(("capacity", [k - 2] + [k] * (n - 1), ring, [0b11111] * n, 1))
    out.append(("min_area", [2] * n, [(1, 0, 0, 0)] * n, [0b11] * n, 3))
    out.append(("self", half, [(b, 1 + b % 3, b, -b) for b in range(n)], ones, 1))
    out.append(("outside", half, [(1, 1, 0, 0), (-1, 3, 2, 2)] + [(n, 0, 0, 0)] * (n - 2), ones, 1))
    out.append(("one_source", [3] * n, [(1, b % 4, b, -2 * b) for b in range(n)], ones, 2))
    out.append(("out_of_frame", half, [((b + 1) % n, 3, (h, -h, 2 ** 31 - 1, -2 ** 31)[b % 4], (0, w, -2 ** 31, 5)[b % 4]) for b in range(n)],
                ones, 1))
    out.append(("empty_batch", [0] * n, ring, ones, 1))
    for t in range(10):                                 # shifts up to the full side, and half of the trials half of that
        ry, rx = (h, w) if t % 2 == 0 else (h // 2, w // 2)
        xform = np.stack([rng.integers(-1, n + 1, n), rng.integers(0, 4, n), rng.integers(-ry, ry + 1, n), rng.integers(-rx, rx + 1, n)], 1)
        out.append(("random%d" % t, rng.integers(0, k + 1, n).tolist(), [tuple(int(v) for v in row) for row in xform],
                    rng.integers(0, 2 ** 32, n, dtype=np.uint64).tolist(), int(rng.integers(1, 8))))
    return out


_REFERENCE = {}


def reference(shape):
    """scene(shape) and, per case, the restatement's outputs: computed once, shared by the tests, never written to."""
    if shape not in _REFERENCE:
        rgb, sem, planes = scene(shape)
        want = {name: CP.copy_paste(rgb, sem, planes, counts, xform, select, min_area)
                for name, counts, xform, select, min_area in cases(shape)}
        for arrays in want.values():
            for a in arrays:
                a.setflags(write=False)
        _REFERENCE[shape] = ((rgb, sem, planes), want)
    return _REFERENCE[shape]


def run(L, lib, shape, dev, counts, xform, select, min_area, poison=0xFF):
    """One call over device inputs `dev`; the outputs and the scratch are filled with `poison` first."""
    n, h, w, k, c = shape
    rgb, sem, planes = dev
    i32 = lambda v, shp: torch.from_numpy((np.asarray(v, np.int64).reshape(shp) & 0xffffffff).astype(np.uint32).view(np.int32)).cuda()
    nobj, xf, sel = i32(counts, (n,)), i32(xform, (n, 4)), i32(select, (n,))
    fill = lambda shp, dt=torch.uint8: torch.full(shp, poison if dt == torch.uint8 else -1 if poison else 0, dtype=dt, device="cuda")
    out = (fill((n, h, w, c)), fill((n, h, w)), fill((n, h, w, k)), fill((n,), torch.int32), fill((n, 4), torch.int32))
    scratch = fill((L.copy_paste_scratch_bytes(n, k),))
    L.check(lib.isa_copy_paste_u8(L.ptr(rgb), L.ptr(sem), L.ptr(planes), L.ptr(nobj), L.ptr(xf), L.ptr(sel), n, h, w, c, k, min_area,
                                  L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]), L.ptr(out[4]), L.ptr(scratch),
                                  scratch.numel(), L.stream_ptr()), "isa_copy_paste_u8")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def same(got, want, what):
    names = ("rgb", "sem", "planes", "n_out", "plan")
    for name, g, w_ in zip(names, got, want):
        if name == "plan":
            g = g.view(np.uint32).astype(np.int64)
        assert g.shape == w_.shape and np.array_equal(g, w_), (what, name)


def check_branches(shape):
    """The branches, on the restatement's plan: they must occur in these inputs before a comparison means anything."""
    n, h, w, k, c = shape
    host, want = reference(shape)
    plans = {name: want[name][4] for name in want}
    counts_of = {name: counts for name, counts, _, _, _ in cases(shape)}
    occ = plans["occlusion"][0]
    assert occ[0] == 0b1 and occ[1] == 0b10 and occ[2] == 2                       # plane 0 dropped, plane 1 moves to the front
    assert any(0 < popcount(p[1]) < counts_of[name][b] and p[0] and p[1] != (1 << popcount(p[1])) - 1
               for name, pl in plans.items() for b, p in enumerate(pl)), "no dropped plane followed by a compaction"
    cap = plans["capacity"][0]
    assert popcount(cap[0]) == 2 and cap[0] == 0b11 and cap[3] == 1 and popcount(cap[1]) + 2 <= k
    assert plans["min_area"][0][0] == 0b01 and plans["min_area"][0][3] == 1      # two pixels are fewer than three
    outside = plans["outside"]
    assert outside[0][0] != 0 and all(p[0] == 0 and p[3] == 0 for p in outside[1:])  # pass-through beside a paste
    assert all(p[0] != 0 for p in plans["one_source"])                            # every target pastes from image 1, itself included
    assert all(p[0] != 0 for p in plans["self"])
    assert all(p[0] == 0 and p[3] == 1 for p in plans["out_of_frame"])
    assert sum(bool(p[0]) for name, pl in plans.items() if name.startswith("random") for p in pl) >= 3


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_restatement(shape):
    L, lib = _lib()
    check_branches(shape)
    host, want = reference(shape)
    dev = tuple(torch.from_numpy(a).cuda() for a in host)
    for name, counts, xform, select, min_area in cases(shape):
        same(run(L, lib, shape, dev, counts, xform, select, min_area), want[name], name)
    assert all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(dev, host))    # the inputs are read only


@pytest.mark.parametrize("shape", SHAPES[:1] + SHAPES[2:], ids=lambda s: "x".join(map(str, s)))
def test_runs_are_identical_whatever_the_scratch_held(shape):
    L, lib = _lib()
    host, want = reference(shape)
    dev = tuple(torch.from_numpy(a).cuda() for a in host)
    for name, counts, xform, select, min_area in cases(shape):
        if name not in ("capacity", "one_source", "random0", "random3"):
            continue
        first = run(L, lib, shape, dev, counts, xform, select, min_area, poison=0xFF)
        second = run(L, lib, shape, dev, counts, xform, select, min_area, poison=0xFF)
        third = run(L, lib, shape, dev, counts, xform, select, min_area, poison=0x00)
        for a, b_, c_ in zip(first, second, third):
            assert np.array_equal(a, b_) and np.array_equal(a, c_), name
        same(first, want[name], name)


def test_host_function_takes_sequences_and_device_tensors():
    L, lib = _lib()
    from isa_amd import data as D
    shape = SHAPES[0]
    n, h, w, k, c = shape
    host, want = reference(shape)
    name, counts, xform, select, min_area = cases(shape)[-1]
    xf = np.asarray(xform)
    got = D.copy_paste(*(torch.from_numpy(a) for a in host), counts, xf[:, 0].tolist(), select, xf[:, 1].tolist(),
                       [tuple(r) for r in xf[:, 2:].tolist()], min_area)
    assert all(t.is_cuda for t in got) and got[3].dtype == torch.int32 and got[4].shape == (n, 4)
    same(tuple(t.cpu().numpy() for t in got), want[name], "sequences")
    t32 = lambda v: torch.from_numpy((np.asarray(v, np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)).cuda()
    got = D.copy_paste(*(torch.from_numpy(a).cuda() for a in host), t32(counts), t32(xf[:, 0]), t32(select), t32(xf[:, 1]), t32(xf[:, 2:]),
                       min_area=min_area)
    same(tuple(t.cpu().numpy() for t in got), want[name], "device tensors")


def test_captured_stage_follows_changed_draws():
    """One stream, no parallel branches: data.copy_paste captured with preallocated outputs and scratch, replayed, then
    xform and select changed in place and replayed again."""
    L, lib = _lib()
    from isa_amd import data as D
    shape = SHAPES[0]
    n, h, w, k, c = shape
    host, want = reference(shape)
    by_name = {name: rest for name, *rest in cases(shape)}
    t32 = lambda v: torch.from_numpy((np.asarray(v, np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)).cuda()
    dev = tuple(torch.from_numpy(a).cuda() for a in host)
    counts, xform, select, min_area = by_name["one_source"]
    nobj, xf, sel = t32(counts), t32(xform), t32(select)
    out = (torch.full((n, h, w, c), 0xFF, dtype=torch.uint8, device="cuda"), torch.full((n, h, w), 0xFF, dtype=torch.uint8, device="cuda"),
           torch.full((n, h, w, k), 0xFF, dtype=torch.uint8, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda"),
           torch.full((n, 4), -1, dtype=torch.int32, device="cuda"))
    scratch = torch.full((L.copy_paste_scratch_bytes(n, k),), 0xFF, dtype=torch.uint8, device="cuda")

    def launch():
        return D.copy_paste(*dev, nobj, xf[:, 0], sel, xf[:, 1], xf[:, 2:], min_area=min_area, out=out, scratch=scratch)
    got = launch()
    torch.cuda.synchronize()
    assert all(a is b_ for a, b_ in zip(got, out))
    same(tuple(t.cpu().numpy() for t in out), want["one_source"], "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for t in out:
        t.fill_(0x5A if t.dtype == torch.uint8 else -7)
    g.replay()
    torch.cuda.synchronize()
    same(tuple(t.cpu().numpy() for t in out), want["one_source"], "first replay")
    for other in ("flips", "random1"):                                    # the same counts are not required: they are an input too
        counts2, xform2, select2, min_area2 = by_name[other]
        if min_area2 != min_area:                                         # min_area travels by value: fixed at capture
            want2 = CP.copy_paste(*host, counts2, xform2, select2, min_area)
        else:
            want2 = want[other]
        nobj.copy_(t32(counts2)), xf.copy_(t32(xform2)), sel.copy_(t32(select2))
        g.replay()
        torch.cuda.synchronize()
        same(tuple(t.cpu().numpy() for t in out), want2, "replay after " + other)
