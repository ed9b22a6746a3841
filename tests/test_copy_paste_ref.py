"""CPU-only: tests/copy_paste_np.py (the oracle of the GPU tests) against hand-written 6 x 8 cases whose expected arrays
are typed out here, and the properties of the contract (include/isa_kernels.h: isa_copy_paste_u8) on random inputs."""
import os
import sys

import numpy as np

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import copy_paste_np as CP   # noqa: E402

H, W = 6, 8


def grid(*rows):
    """Six strings of eight characters: a digit is that byte value, '.' is 0."""
    assert len(rows) == H and all(len(r) == W for r in rows), rows
    return np.array([[0 if ch == '.' else int(ch) for ch in r] for r in rows], np.uint8)


EMPTY = grid("........", "........", "........", "........", "........", "........")
ONES = grid("11111111", "11111111", "11111111", "11111111", "11111111", "11111111")
# image 0, the target: two instances (byte values 1 and 2)
T0 = grid("11......", "11......", "........", "........", "........", "........")
T1 = grid("........", "........", "........", "...22...", "...22...", "........")
T_SEM = grid("11......", "11......", "........", "...11...", "...11...", "........")
# image 1, the source: two instances (byte values 5 and 9), an image in which every row differs
S0 = grid("........", ".55.....", ".55.....", ".5......", "........", "........")
S1 = grid("......99", "......99", "........", "........", "........", "........")
S_SEM = grid("......33", ".33...33", ".33.....", ".3......", "........", "........")
S_RGB = grid("01234567", "89012345", "67890123", "45678901", "23456789", "01234567")


def batch(k=4, source_garbage=False):
    planes = np.zeros((2, H, W, k), np.uint8)
    planes[0, :, :, 0], planes[0, :, :, 1], planes[1, :, :, 0], planes[1, :, :, 1] = T0, T1, S0, S1
    if source_garbage:
        planes[1, :, :, 2:] = 255                       # at and beyond n_objects[1]: never read
        planes[0, :, :, 3] = 77                         # beyond n_objects[0]: replaced by a pasted or a zero plane
    rgb = np.stack([ONES, S_RGB])[..., None].repeat(3, 3)
    rgb[..., 1] += 100                                  # three channels that differ
    rgb[..., 2] += 200
    return rgb, np.stack([T_SEM, S_SEM]), planes, [2, 2]


def run(xform0, select0, min_area=1, **kw):
    """Image 0 receives the paste; image 1 has src = -1.  Returns image 0's (rgb channel 0, sem, planes, n_out, plan)."""
    rgb, sem, planes, counts = batch(**kw)
    r, s, p, n_out, plan = CP.copy_paste(rgb, sem, planes, counts, [xform0, (-1, 3, 1, 1)], [select0, 0xffffffff], min_area)
    assert np.array_equal(r[..., 1], r[..., 0] + 100) and np.array_equal(r[..., 2], r[..., 0] + 200)
    # image 1 passes through (its planes beyond the count zeroed)
    want = planes[1].copy()
    want[:, :, 2:] = 0
    assert np.array_equal(r[1], rgb[1]) and np.array_equal(s[1], sem[1]) and np.array_equal(p[1], want)
    assert n_out[1] == 2 and plan[1].tolist() == [0, 0b11, 2, 0]
    assert n_out.dtype == np.int32 and p.dtype == r.dtype == s.dtype == np.uint8
    return r[0, :, :, 0], s[0], p[0], int(n_out[0]), plan[0].tolist()


def check_planes(got, *want):
    for i in range(got.shape[2]):
        assert np.array_equal(got[:, :, i], want[i] if i < len(want) else EMPTY), i


def test_paste_without_flip_or_shift():
    for garbage in (False, True):                       # garbage behind the counts changes nothing
        r, s, p, n_out, plan = run((1, 0, 0, 0), 0xffffffff if garbage else 0b11, source_garbage=garbage)
        assert np.array_equal(r, grid("11111167", "19011145", "17811111", "15111111", "11111111", "11111111"))
        assert np.array_equal(s, grid("11....33", "133...33", ".33.....", ".3.11...", "...11...", "........"))
        check_planes(p, grid("11......", "1.......", "........", "........", "........", "........"), T1, S0, S1)
        assert n_out == 4 and plan == [0b11, 0b11, 4, 0]


def test_flip_along_x():
    r, s, p, n_out, plan = run((1, 1, 0, 0), 0b01)
    assert np.array_equal(r, grid("11111111", "11111091", "11111871", "11111151", "11111111", "11111111"))
    assert np.array_equal(s, grid("11......", "11...33.", ".....33.", "...11.3.", "...11...", "........"))
    check_planes(p, T0, T1, grid("........", ".....55.", ".....55.", "......5.", "........", "........"))
    assert n_out == 3 and plan == [0b01, 0b11, 3, 0]


def test_flip_along_y():
    r, s, p, n_out, plan = run((1, 2, 0, 0), 0b01)
    assert np.array_equal(r, grid("11111111", "11111111", "15111111", "17811111", "19011111", "11111111"))
    assert np.array_equal(s, grid("11......", "11......", ".3......", ".3311...", ".3311...", "........"))
    check_planes(p, T0, T1, grid("........", "........", ".5......", ".55.....", ".55.....", "........"))
    assert n_out == 3 and plan == [0b01, 0b11, 3, 0]


def test_both_flips():
    r, s, p, n_out, plan = run((1, 3, 0, 0), 0b01)
    assert np.array_equal(r, grid("11111111", "11111111", "11111151", "11111871", "11111091", "11111111"))
    check_planes(p, T0, T1, grid("........", "........", "......5.", ".....55.", ".....55.", "........"))
    assert n_out == 3 and plan == [0b01, 0b11, 3, 0]


def test_full_occlusion_drops_the_target_plane_and_compacts():
    r, s, p, n_out, plan = run((1, 1, 0, 0), 0b10)      # the source's second instance, mirrored, lies on the target's first
    assert np.array_equal(r, grid("76111111", "54111111", "11111111", "11111111", "11111111", "11111111"))
    assert np.array_equal(s, grid("33......", "33......", "........", "...11...", "...11...", "........"))
    check_planes(p, T1, grid("99......", "99......", "........", "........", "........", "........"))
    assert n_out == 2 and plan == [0b10, 0b10, 2, 0]


def test_shift_cuts_an_object_at_the_border_and_min_area_refuses_it():
    r, s, p, n_out, plan = run((1, 0, -1, 1), 0b11)     # up by one, right by one: one pixel of the second instance is left
    assert np.array_equal(r, grid("11901114", "11781111", "11511111", "11111111", "11111111", "11111111"))
    assert np.array_equal(s, grid("1133...3", "1133....", "..3.....", "...11...", "...11...", "........"))
    check_planes(p, T0, T1, grid("..55....", "..55....", "..5.....", "........", "........", "........"),
                 grid(".......9", "........", "........", "........", "........", "........"))
    assert n_out == 4 and plan == [0b11, 0b11, 4, 0]
    r, s, p, n_out, plan = run((1, 0, -1, 1), 0b11, min_area=2)
    assert np.array_equal(r, grid("11901111", "11781111", "11511111", "11111111", "11111111", "11111111"))
    assert np.array_equal(s, grid("1133....", "1133....", "..3.....", "...11...", "...11...", "........"))
    check_planes(p, T0, T1, grid("..55....", "..55....", "..5.....", "........", "........", "........"))
    assert n_out == 3 and plan == [0b01, 0b11, 3, 1]
    for min_area in (0, -5):                            # values below 1 mean 1
        assert run((1, 0, -1, 1), 0b11, min_area=min_area)[4] == [0b11, 0b11, 4, 0]
    # a shift that leaves nothing in frame pastes nothing, and neither does an instance that is not selected
    for xform in ((1, 0, H, 0), (1, 0, 0, -W), (1, 3, 2 ** 31 - 1, -2 ** 31)):
        r, s, p, n_out, plan = run(xform, 0b11)
        assert np.array_equal(r, ONES) and np.array_equal(s, T_SEM) and n_out == 2 and plan == [0, 0b11, 2, 1]
        check_planes(p, T0, T1)
    assert run((1, 0, 0, 0), 0b100)[4] == [0, 0b11, 2, 0]


def test_capacity_takes_the_first_candidates():
    k = 8
    planes = np.zeros((2, H, W, k), np.uint8)
    for i in range(6):
        planes[0, 5, i, i] = 1                          # six target instances of one pixel in the last row
    for j in range(5):
        planes[1, 0, j, j] = j + 2                      # five source instances of one pixel in the first row
    rgb = np.stack([ONES, S_RGB])[..., None]
    sem = np.stack([grid("........", "........", "........", "........", "........", "111111.."),
                    grid("33333...", "........", "........", "........", "........", "........")])
    r, s, p, n_out, plan = CP.copy_paste(rgb, sem, planes, [6, 5], [(1, 0, 0, 0), (-1, 0, 0, 0)], [0b11111, 0])
    assert np.array_equal(r[0, :, :, 0], grid("01111111", "11111111", "11111111", "11111111", "11111111", "11111111"))
    assert np.array_equal(s[0], grid("33......", "........", "........", "........", "........", "111111.."))
    want = planes[0].copy()
    want[0, 0, 6], want[0, 1, 7] = 2, 3
    assert np.array_equal(p[0], want)
    assert n_out.tolist() == [8, 5] and plan.tolist() == [[0b00011, 0b111111, 8, 1], [0, 0b11111, 5, 0]]
    # a full target takes nothing and, passing through, keeps its two empty planes
    r, s, p, n_out, plan = CP.copy_paste(rgb, sem, planes, [8, 5], [(1, 0, 0, 0), (-1, 0, 0, 0)], [0b11111, 0])
    assert plan[0].tolist() == [0, 0xff, 8, 1] and np.array_equal(p[0], planes[0]) and np.array_equal(r[0], rgb[0])
    # one plane free: the first SELECTED candidate takes it; the target's empty seventh plane is dropped now (the capacity
    # was counted before, so the eighth slot stays free)
    r, s, p, n_out, plan = CP.copy_paste(rgb, sem, planes, [7, 5], [(1, 0, 0, 0), (-1, 0, 0, 0)], [0b11010, 0])
    assert plan[0].tolist() == [0b00010, 0x3f, 7, 1] and p[0, 0, 1, 6] == 3 and np.count_nonzero(p[0, :, :, 6:]) == 1
    assert np.array_equal(p[0, :, :, :6], planes[0, :, :, :6])


def test_an_image_pasted_onto_itself():
    r, s, p, n_out, plan = run((0, 1, 0, 0), 0b11)      # mirrored: the first instance lands in the other corner, the second on itself
    assert np.array_equal(r, ONES)
    assert np.array_equal(s, grid("11....11", "11....11", "........", "...11...", "...11...", "........"))
    check_planes(p, T0, grid("......11", "......11", "........", "........", "........", "........"), T1)
    assert n_out == 3 and plan == [0b11, 0b01, 3, 0]


def test_sources_outside_the_batch_pass_through():
    for src in (-1, 2, 7, -2 ** 31):
        r, s, p, n_out, plan = run((src, 1, 1, 1), 0xffffffff, source_garbage=True)
        assert np.array_equal(r, ONES) and np.array_equal(s, T_SEM) and n_out == 2 and plan == [0, 0b11, 2, 0]
        check_planes(p, T0, T1)


def _random_batch(rng, n, h, w, k, c, values):
    planes = np.zeros((n, h, w, k), np.uint8)
    counts = rng.integers(0, k + 1, n)
    for b in range(n):
        for i in range(k):                              # small and large instances; planes behind the count hold garbage
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            hh, ww = (rng.integers(1, 3), rng.integers(1, 3)) if rng.random() < 0.5 else (rng.integers(1, h), rng.integers(1, w))
            planes[b, y0:y0 + hh, x0:x0 + ww, i] = values[rng.integers(len(values))]
    xform = np.stack([rng.integers(-1, n + 1, n), rng.integers(0, 4, n), rng.integers(-h // 2, h // 2 + 1, n),
                      rng.integers(-w // 2, w // 2 + 1, n)], 1)
    return (rng.integers(0, 256, (n, h, w, c), dtype=np.uint8), rng.integers(0, 256, (n, h, w), dtype=np.uint8), planes, counts,
            xform, rng.integers(0, 2 ** 32, n, dtype=np.uint64))


def test_properties_on_random_inputs():
    rng = np.random.default_rng(5)
    seen = dict(paste=0, drop=0, flag=0, through=0)
    for trial in range(80):
        n, h, w, k, c = 3, int(rng.integers(3, 12)), int(rng.integers(3, 12)), int(rng.integers(1, 9)), int(rng.integers(1, 5))
        rgb, sem, planes, counts, xform, select = _random_batch(rng, n, h, w, k, c, (1, 7, 255))
        min_area = int(rng.integers(0, 4))
        r, s, p, n_out, plan = CP.copy_paste(rgb, sem, planes, counts, xform, select, min_area)
        for b in range(n):
            pasted, kept, count, flag = (int(v) for v in plan[b])
            nb = int(counts[b])
            assert count == n_out[b] == bin(kept).count("1") + bin(pasted).count("1") <= k
            assert not p[b, :, :, count:].any()                          # zero planes behind the count
            assert kept < (1 << nb) and (pasted == 0 or 0 <= xform[b, 0] < n and pasted < (1 << int(counts[xform[b, 0]])))
            assert pasted & ~int(select[b]) == 0
            # M is where the image or the semantic map may have changed; elsewhere the outputs equal the inputs
            kept_list = [i for i in range(nb) if (kept >> i) & 1]
            if not pasted:
                assert kept_list == list(range(nb)) and np.array_equal(p[b, :, :, :nb], planes[b, :, :, :nb])
                assert np.array_equal(r[b], rgb[b]) and np.array_equal(s[b], sem[b])
                seen["through"] += 1
                seen["flag"] += flag
                continue
            seen["paste"] += 1
            seen["drop"] += len(kept_list) < nb
            seen["flag"] += flag
            new = p[b, :, :, len(kept_list):count]
            m = (new != 0).any(2)
            assert m.any() and all(np.count_nonzero(new[:, :, o]) >= max(min_area, 1) for o in range(new.shape[2]))
            assert np.array_equal(r[b][~m], rgb[b][~m]) and np.array_equal(s[b][~m], sem[b][~m])
            for o, i in enumerate(kept_list):                            # a kept plane: its bytes outside M, zero inside, not empty
                assert np.array_equal(p[b, :, :, o][~m], planes[b, :, :, i][~m]) and not p[b, :, :, o][m].any() and p[b, :, :, o].any()
            for i in set(range(nb)) - set(kept_list):                    # a dropped plane had nothing outside M
                assert not planes[b, :, :, i][~m].any()
            assert set(np.unique(new)) <= {0, 1, 7, 255}                 # byte values survive
    assert min(seen.values()) >= 5, seen
    assert {7, 255} <= set(np.unique(p))


def test_byte_values_are_carried_through():
    rgb, sem, planes, counts = batch()
    planes[1, :, :, 0] = np.where(S0 != 0, 255, 0)
    planes[0, :, :, 1] = np.where(T1 != 0, 7, 0)
    r, s, p, n_out, plan = CP.copy_paste(rgb, sem, planes, counts, [(1, 0, 0, 0), (-1, 0, 0, 0)], [0b01, 0])
    assert np.array_equal(p[0, :, :, 1], np.where(T1 != 0, 7, 0)) and np.array_equal(p[0, :, :, 2], np.where(S0 != 0, 255, 0))
