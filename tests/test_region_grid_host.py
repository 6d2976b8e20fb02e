"""CPU: the region grids the library chooses per launch for the three encoder window kernels (csrc/msda_grid.h region_grid_choice),
through semidetr_msda_region_grid_query -- no GPU.  The kernels' query -> region map (msda_rw.h / msda_gw.h / msda_region.h: even
tiling of the finest level, a level-l pixel belongs to the region its centre maps into) is restated here from the level table and
must cover every pixel of every level exactly once for every grid a test pins."""
import numpy as np
import pytest

import semi_detr_amd as sda

FULL4 = [(100, 167), (50, 84), (25, 42), (13, 21)]          # the 800 x 1333 pyramid
FULL5 = FULL4 + [(7, 11)]
SMALL4 = [(9, 13), (5, 7), (3, 4), (2, 2)]
SMALL5 = SMALL4 + [(1, 1)]
CUS, HEADS = 256, 8
KERNELS = ("forward", "gather", "scatter")


def largest_region(kernel, levels):
    """(RTH, RTW) the kernel's windows are sized for (csrc/msda_tuning.h: SEMIDETR_RW_RTH / _RTH5, SEMIDETR_GW_RTH / _RTH5, SEMIDETR_SCATTER_RTH / _RTW)"""
    five = len(levels) == 5
    return {"forward": (24 if five else 25, 16), "gather": (13 if five else 15, 16), "scatter": (8, 24)}[kernel]


def coarsest(kernel, levels):
    rth, rtw = largest_region(kernel, levels)
    h0, w0 = grid_level(kernel, levels)
    return -(-h0 // rth), -(-w0 // rtw)


def grid_level(kernel, levels):
    """the level that carries the grid: level 0 for the window kernels, the one with the most pixels for the scatter"""
    return levels[0] if kernel != "scatter" else max(levels, key=lambda hw: hw[0] * hw[1])


def first(bound, nq, nb):
    """smallest q in [0, nq] whose pixel centre maps into row >= bound of the nb-row grid level: ((2 q + 1) nb) // (2 nq) >= bound"""
    return min(nq, ((2 * nq * bound + nb - 1) // nb) >> 1)


def region_rectangles(kernel, levels, nry, nrx, even=True):
    """per region a list over levels of (ylo, yhi, xlo, xhi); even: balanced tiling, else steps of RTH x RTW (the scatter's own grid)"""
    hb, wb = grid_level(kernel, levels)
    rth, rtw = largest_region(kernel, levels)
    out = []
    for ry in range(nry):
        for rx in range(nrx):
            y0, y1 = (ry * hb // nry, (ry + 1) * hb // nry) if even else (ry * rth, min(ry * rth + rth, hb))
            x0, x1 = (rx * wb // nrx, (rx + 1) * wb // nrx) if even else (rx * rtw, min(rx * rtw + rtw, wb))
            rects = []
            for h, w in levels:
                ylo, yhi = first(y0, h, hb), (h if y1 >= hb else first(y1, h, hb))
                xlo, xhi = first(x0, w, wb), (w if x1 >= wb else first(x1, w, wb))
                rects.append((ylo, max(yhi, ylo), xlo, max(xhi, xlo)))
            out.append(rects)
    return out


def pinned_grids(kernel, levels):
    """the grids the GPU test pins: the coarsest, + 1 in each axis (uneven tiles), one-row regions, more columns than pixels"""
    ny0, nx0 = coarsest(kernel, levels)
    h0, w0 = grid_level(kernel, levels)
    return {"coarsest": (ny0, nx0), "plus_one": (ny0 + 1, nx0 + 1), "one_row": (h0, nx0), "no_pixel": (ny0, w0 + 2)}


@pytest.fixture(autouse=True)
def _unpinned():
    yield
    for k in KERNELS:
        sda._lib.set_region_grid(k, 0, 0)


@pytest.mark.parametrize("levels", [FULL4, FULL5], ids=["four_levels", "five_levels"])
@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("kernel", KERNELS)
def test_chosen_grid_respects_the_windows_and_sizes_the_launch_exactly(kernel, batch, levels):
    g = sda._lib.region_grid(kernel, levels, batch, HEADS, CUS)
    ny0, nx0 = coarsest(kernel, levels)
    nry, nrx = (g["nry"], g["nrx"]) if g["nry"] else (ny0, nx0)          # 0, 0: the kernel's own coarsest grid
    assert (g["nry"] == 0) == (g["nrx"] == 0)
    assert nry >= ny0 and nrx >= nx0, (g, ny0, nx0)
    assert g["regions"] == nry * nrx and g["workgroups"] == batch * g["regions"] * HEADS, g
    rects = region_rectangles(kernel, levels, nry, nrx, even=g["nry"] != 0 or kernel != "scatter")
    assert g["max_queries"] == max(sum((b - a) * (d - c) for a, b, c, d in r) for r in rects)
    rth, rtw = largest_region(kernel, levels)
    lb = levels.index(grid_level(kernel, levels))
    assert all(r[lb][1] - r[lb][0] <= rth and r[lb][3] - r[lb][2] <= rtw for r in rects)
    # the same question twice is the same answer (the choice is cached per table, batch, heads, kernel)
    assert sda._lib.region_grid(kernel, levels, batch, HEADS, CUS) == g


def test_one_image_fills_whole_waves_and_four_images_keep_the_coarsest_grid():
    """what the sweep on the device decided (profiles/region_grid_probe.txt): one image gets a finer grid for the window forward and the
    window gather; four images, and the scatter at either size, keep the coarsest"""
    one = {k: sda._lib.region_grid(k, FULL4, 1, HEADS, CUS) for k in KERNELS}
    assert (one["forward"]["nry"], one["forward"]["nrx"]) == (4, 16) and one["forward"]["workgroups"] == 2 * CUS
    assert one["forward"]["tail_split"] == 0
    assert (one["gather"]["nry"], one["gather"]["nrx"]) == (8, 12) and one["gather"]["workgroups"] == 3 * CUS
    four = {k: sda._lib.region_grid(k, FULL4, 4, HEADS, CUS) for k in KERNELS}
    assert (four["forward"]["nry"], four["forward"]["nrx"]) == coarsest("forward", FULL4)
    assert (four["gather"]["nry"], four["gather"]["nrx"]) == coarsest("gather", FULL4)
    for g in (one["scatter"], four["scatter"]):
        assert (g["nry"], g["nrx"]) == (0, 0) and g["regions"] == 13 * 7


@pytest.mark.parametrize("kernel", KERNELS)
def test_without_a_table_the_answer_is_default(kernel):
    assert sda._lib.region_grid(kernel, None, 4, HEADS, CUS) == dict(nry=0, nrx=0, regions=0, workgroups=0, tail_split=0, max_queries=0)
    # a level beyond what the window kernels' 15-bit pixel fields take counts as no table
    g = sda._lib.region_grid(kernel, [(40000, 3), (20000, 2)], 1, HEADS, CUS)
    assert g["regions"] == 0 and g["nry"] == 0
    # no compute-unit count (a device that will not say): no choice either
    assert sda._lib.region_grid(kernel, FULL4, 1, HEADS, 0)["regions"] == 0


def test_pin_arguments_are_validated():
    lib = sda._lib.lib()
    assert lib.semidetr_msda_set_region_grid(3, 1, 1) == -1 and b"0 forward" in lib.semidetr_last_error()
    assert lib.semidetr_msda_set_region_grid(0, 1, 0) == -1
    assert lib.semidetr_msda_set_region_grid(0, -1, -1) == -1
    assert lib.semidetr_msda_set_region_grid(0, 2, 3) == 0 and lib.semidetr_msda_set_region_grid(0, 0, 0) == 0
    assert lib.semidetr_msda_region_grid_query(0, None, 4, 1, 8, 256, None) == -1


@pytest.mark.parametrize("levels", [SMALL4, SMALL5, FULL4, FULL5], ids=["small4", "small5", "full4", "full5"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_every_pixel_of_every_level_belongs_to_exactly_one_region(kernel, levels):
    for name, (ny, nx) in pinned_grids(kernel, levels).items():
        sda._lib.set_region_grid(kernel, ny, nx)
        g = sda._lib.region_grid(kernel, levels, 2, 2, CUS)
        assert (g["nry"], g["nrx"]) == (ny, nx) and g["regions"] == ny * nx and g["workgroups"] == 2 * ny * nx * 2, (name, g)
        # ... and a pin without a table reaches the kernel as it is, the grid size stays a hint
        assert sda._lib.region_grid(kernel, None, 2, 2, CUS) == dict(nry=ny, nrx=nx, regions=0, workgroups=0, tail_split=0, max_queries=0)
        rects = region_rectangles(kernel, levels, ny, nx)
        seen = [np.zeros(hw, np.int32) for hw in levels]
        for r in rects:
            for lvl, (a, b, c, d) in enumerate(r):
                seen[lvl][a:b, c:d] += 1
        assert all((s == 1).all() for s in seen), (kernel, name, [np.argwhere(s != 1)[:3].tolist() for s in seen])
        assert g["max_queries"] == max(sum((b - a) * (d - c) for a, b, c, d in r) for r in rects), (name, g)
        rth, rtw = largest_region(kernel, levels)
        lb = levels.index(grid_level(kernel, levels))
        assert all(r[lb][1] - r[lb][0] <= rth and r[lb][3] - r[lb][2] <= rtw for r in rects), name
    # a pin coarser than the windows allow is raised to the coarsest grid
    sda._lib.set_region_grid(kernel, 1, 1)
    g = sda._lib.region_grid(kernel, levels, 2, 2, CUS)
    assert (g["nry"], g["nrx"]) == coarsest(kernel, levels)
    # the scatter's own grid (no pin): steps of 8 x 24 pixels, the remainder at the bottom / right edge -- covers every pixel once too
    if kernel == "scatter":
        ny0, nx0 = coarsest(kernel, levels)
        seen = [np.zeros(hw, np.int32) for hw in levels]
        for r in region_rectangles(kernel, levels, ny0, nx0, even=False):
            for lvl, (a, b, c, d) in enumerate(r):
                seen[lvl][a:b, c:d] += 1
        assert all((s == 1).all() for s in seen)
