"""No GPU: the plan of the depthwise rows kernels (yolo_dw_plan, csrc/dwconv.hip) over the seven depthwise layers of preset s
at 32 images and the small shapes of tests/test_gpu_dw_rows.py.  The walk is replayed on the host exactly as the kernels
decode it (item -> image, band, column block; thread -> column), so "every pixel once" is a statement about the plan
values the launch uses."""
import numpy as np
import pytest

from src.hipops import lib

WORKLOAD = [(32, 128, 80, 80), (32, 256, 40, 40), (32, 128, 40, 40), (32, 512, 20, 20), (32, 128, 20, 20)]   # (N, C, H, W)
SMALL = [(3, 16, 1, 6), (3, 16, 2, 6), (3, 16, 3, 6), (3, 16, 7, 6), (3, 16, 37, 6), (3, 16, 5, 1), (3, 16, 5, 5),
         (3, 128, 5, 21), (3, 128, 5, 20), (3, 8, 5, 6), (3, 24, 6, 7), (3, 136, 5, 6), (3, 2056, 3, 5)]
FIELDS = ("kernel", "ncol", "ncb", "cvb", "wg", "hb", "nb", "grid", "hb_wg", "nb_wg", "grid_wg", "ncy")


def plan(n, c, h, w, variant=2):
    """the plan with the rows kernels forced (2), or as the launcher chooses (0)"""
    lib.call("yolo_dw_tune_set", variant)
    try:
        p = {k: lib.query("yolo_dw_plan", n, h, w, c, i) for i, k in enumerate(FIELDS)}
        p["kernel_wgrad"] = lib.query("yolo_dw_plan", n, h, w, c, 12)
        return p
    finally:
        lib.call("yolo_dw_tune_set", 0)


def coverage(n, h, w, p, hb, nb, grid):
    """times each (image, row, column) is written when `grid` workgroups walk the items of the plan"""
    seen = np.zeros((n, h, w), dtype=np.int32)
    total = n * nb * p["ncb"]
    for wgx in range(grid):
        for s in range(wgx, total, grid):
            cbk, t2 = s % p["ncb"], s // p["ncb"]
            band, img = t2 % nb, t2 // nb
            h0 = band * hb
            h1 = min(h0 + hb, h)
            for col in range(p["ncol"]):
                wc = cbk * p["ncol"] + col
                if wc < w:
                    seen[img, h0:h1, wc] += 1
    return seen


@pytest.mark.parametrize("n,c,h,w", WORKLOAD + SMALL)
def test_items_cover_every_pixel_once(n, c, h, w):
    p = plan(n, c, h, w)
    assert p["kernel"] == 1, p
    assert p["cvb"] == min(c // 8, 256) and p["ncy"] == -(-(c // 8) // p["cvb"])
    assert 1 <= p["ncol"] <= w and p["cvb"] * p["ncol"] <= p["wg"] <= 256 and p["wg"] % 64 == 0, p
    assert p["ncb"] == -(-w // p["ncol"])
    for hb, nb, grid in ((p["hb"], p["nb"], p["grid"]), (p["hb_wg"], p["nb_wg"], p["grid_wg"])):
        assert hb >= 1 and nb == -(-h // hb) and 1 <= grid <= n * nb * p["ncb"], p
        seen = coverage(n, h, w, p, hb, nb, grid)
        assert seen.min() == 1 and seen.max() == 1, (p, int(seen.min()), int(seen.max()))


@pytest.mark.parametrize("n,c,h,w", WORKLOAD + SMALL)
def test_idle_columns_at_most_a_quarter(n, c, h, w):
    p = plan(n, c, h, w)
    slots = p["ncb"] * p["ncol"]
    assert 4 * (slots - w) <= slots, p


def test_replanned_columns_on_20_wide_maps():
    """20 columns x 16 channel groups: 10 + 10 columns, not 16 + 4"""
    assert plan(32, 128, 20, 20)["ncol"] in (10, 20)


@pytest.mark.parametrize("n,c,h,w", [s for s in WORKLOAD if s[2] >= 40])
def test_two_workgroups_per_cu_on_the_large_maps(n, c, h, w):
    p = plan(n, c, h, w)
    assert p["nb"] * p["ncb"] * n >= 2 * 256, p
    assert p["grid"] * p["ncy"] >= 2 * 256, p


@pytest.mark.parametrize("n,c,h,w", WORKLOAD + SMALL)
def test_wgrad_grid_fits_the_partial_buffer(n, c, h, w):
    p = plan(n, c, h, w)
    assert 1 <= p["grid_wg"] <= lib.query("yolo_dw_wgrad_nslab", n, h), p


def test_the_launcher_chooses_per_shape():
    """forward / data gradient walk rows on the maps measured ahead (16 MiB and more), the weight gradient everywhere; the
    two forced settings hold for every shape"""
    for n, c, h, w in WORKLOAD + SMALL:
        p = plan(n, c, h, w, variant=0)
        assert p["kernel"] == (1 if n * c * h * w * 2 >= 16 << 20 else 2) and p["kernel_wgrad"] == 1, (n, c, h, w, p)
        p = plan(n, c, h, w, variant=1)
        assert p["kernel"] == 2 and p["kernel_wgrad"] == 2
        p = plan(n, c, h, w, variant=2)
        assert p["kernel"] == 1 and p["kernel_wgrad"] == 1
    assert plan(32, 128, 80, 80, 0)["kernel"] == 1 and plan(32, 256, 40, 40, 0)["kernel"] == 1 and plan(32, 128, 40, 40, 0)["kernel"] == 2


def test_shapes_without_a_plan():
    assert lib.query("yolo_dw_plan", 2, 5, 6, 12, 0) == 0          # 12 channels: the generic kernels
    assert lib.query("yolo_dw_plan", 0, 5, 6, 16, 0) == -1
