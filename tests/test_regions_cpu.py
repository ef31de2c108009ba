"""The flood regions' semantics without a device: the numpy oracle (tests/regions_oracle.py) against scipy.ndimage and
hand-checked cases, the option refusals, the exports and the CSV."""
import numpy as np
import pytest

import regions_oracle as RO

SHAPES = [(1, 1), (1, 37), (37, 1), (16, 16), (41, 53), (96, 130)]
STRUCTURES = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1], [1, 1, 1], [1, 1, 1]]}


def _grid(rows):
    return np.array([[c == "#" for c in r] for r in rows])


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SHAPES)
def test_oracle_labels_match_scipy(H, W, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, make in RO.PATTERNS.items():
        mask = make(H, W)
        got = RO.label(mask, connectivity)
        lab, n = ndimage.label(mask, structure=STRUCTURES[connectivity])
        assert np.array_equal(got >= 0, mask), name
        if n == 0:
            assert (got == -1).all(), name
            continue
        index = np.arange(H * W).reshape(H, W)
        first = np.asarray(ndimage.minimum(index, lab, np.arange(1, n + 1))).astype(np.int64).reshape(-1)
        want = np.where(mask, first[np.maximum(lab, 1) - 1], -1)
        assert np.array_equal(got, want), (name, H, W, connectivity)
        assert len(np.unique(got[got >= 0])) == n


def test_the_issue_s_prototype_numbers():
    """96 x 130 Bernoulli(0.593) at 4-connectivity is near the percolation threshold: hundreds of components, one
    of which spans the scene; the sieve at 8 / 8 removes most of them and fills many holes"""
    mask = RO.PATTERNS["bernoulli_0.593"](96, 130)
    tab = RO.table(RO.label(mask, 4))
    big = int(np.argmax(tab["area"]))
    assert len(tab["label"]) > 200 and tab["area"][big] > 1000
    assert tab["y1"][big] - tab["y0"][big] >= 48
    res = RO.flood_regions(mask, 8, 8, 4)
    assert res["removed"] > 100 and res["filled"] > 50 and res["count"] < len(tab["label"]) - res["removed"] + 1


def test_patterns_are_what_they_claim():
    for H, W in [(16, 16), (41, 53), (96, 130)]:
        for c in (4, 8):
            assert len(np.unique(RO.label(RO.spiral(H, W), c))) == 2                # -1 and one label
            assert len(np.unique(RO.label(RO.serpentine(H, W), c))) == 2
        assert RO.spiral(H, W).sum() > H * W // 2 - H - W
        cb = RO.checkerboard(H, W)
        assert len(np.unique(RO.label(cb, 8))) == 2
        assert len(np.unique(RO.label(cb, 4))) == 1 + (H * W + 1) // 2
        assert len(np.unique(RO.label(RO.stripes(H, W, True), 8))) == 1 + (W + 1) // 2
        assert len(np.unique(RO.label(RO.frame_island(H, W), 8))) == 3


def test_diagonal_pair_is_one_region_at_8_and_two_at_4():
    m = _grid([".....",
               ".#...",
               "..#..",
               ".....",
               "....."])
    assert RO.label(m, 8)[2, 2] == 6 and RO.label(m, 8)[1, 1] == 6
    assert RO.label(m, 4)[1, 1] == 6 and RO.label(m, 4)[2, 2] == 12
    t8, t4 = RO.table(RO.label(m, 8)), RO.table(RO.label(m, 4))
    assert {k: v.tolist() for k, v in t8.items()} == {"label": [6], "area": [2], "y0": [1], "x0": [1], "y1": [2],
                                                      "x1": [2], "sum_y": [3], "sum_x": [3]}
    assert t4["label"].tolist() == [6, 12] and t4["area"].tolist() == [1, 1]


RING = [".....",
        ".###.",
        ".#.#.",
        ".###.",
        "....."]


def test_a_ring_s_hole_is_filled():
    for c in (4, 8):
        res = RO.flood_regions(_grid(RING), 1, 2, c)
        assert res["filled"] == 1 and res["removed"] == 0 and res["count"] == 1
        assert np.array_equal(res["mask"], _grid([".....", ".###.", ".###.", ".###.", "....."]))
        assert res["table"]["area"].tolist() == [9] and res["centroids"].tolist() == [[2.0, 2.0]]
        assert res["flood_fraction"] == 9 / 25
        # a hole of area 1 is not below min_hole 1
        assert RO.flood_regions(_grid(RING), 1, 1, c)["filled"] == 0


def test_a_ring_opened_to_the_border_is_not_filled():
    m = _grid([".....",
               ".#.#.",                # the opening: the inner column reaches row 0
               ".#.#.",
               ".###.",
               "....."])
    for c in (4, 8):
        res = RO.flood_regions(m, 1, 1000, c)
        assert res["filled"] == 0 and np.array_equal(res["mask"], m)
    # ... and an enclosed lake that the border does not touch is, whatever its size below the minimum
    closed = m.copy()
    closed[0, 1:4] = True
    res = RO.flood_regions(closed, 1, 1000, 8)
    assert res["filled"] == 1 and res["mask"][1, 2] and res["mask"][2, 2]


def test_a_hole_that_leaks_diagonally_is_outside_when_flood_is_4_connected():
    m = _grid([".....",
               ".##..",
               ".#.#.",
               ".###.",
               "....."])
    # flood at 4: the dry class is 8-connected, (2, 2) touches (1, 3) diagonally and so the outside: not a hole
    res4 = RO.flood_regions(m, 1, 5, 4)
    assert res4["filled"] == 0 and np.array_equal(res4["mask"], m)
    # flood at 8: the dry class is 4-connected, the diagonal does not leak: the hole is filled
    res8 = RO.flood_regions(m, 1, 5, 8)
    assert res8["filled"] == 1 and res8["mask"][2, 2] and res8["mask"].sum() == m.sum() + 1


def test_removal_runs_before_filling_and_filled_holes_join_regions():
    m = _grid(["#######",
               "#.....#",
               "#.#.#.#",
               "#.....#",
               "#######"])
    # the two specks go first, which turns the lake into one hole of 15 pixels; min_hole 16 then fills it
    res = RO.flood_regions(m, 2, 16, 8)
    assert res["removed"] == 2 and res["filled"] == 1 and res["mask"].all() and res["count"] == 1
    assert res["table"]["area"].tolist() == [35]
    # without the removal the lake (13 pixels, the islands kept) is filled and the islands join the frame
    res = RO.flood_regions(m, 1, 16, 8)
    assert res["removed"] == 0 and res["filled"] == 1 and res["mask"].all()


def test_option_refusals_come_before_any_launch():
    import torch

    from floodgan.regions import flood_regions, label_regions
    cpu = torch.zeros(4, 4)
    with pytest.raises(ValueError, match="connectivity must be 4 or 8 \\(got 6\\)"):
        label_regions(cpu, connectivity=6)
    with pytest.raises(ValueError, match="min_region -1"):
        flood_regions(cpu, min_region=-1)
    with pytest.raises(ValueError, match="min_hole -3"):
        flood_regions(cpu, min_hole=-3)
    with pytest.raises(ValueError, match="kind must be one of"):
        flood_regions(cpu, kind="unit")
    with pytest.raises(ValueError, match="float32 tensor on a HIP device"):
        flood_regions(cpu)
    with pytest.raises(ValueError, match="float32 tensor on a HIP device"):
        label_regions(np.zeros((4, 4), np.float32))


def test_predict_scene_refuses_minima_without_a_segmentation_model():
    import torch

    from floodgan.scene import predict_scene

    class Cuda(torch.Tensor):                    # passes require_device without a device
        is_cuda = True

    x = torch.zeros(1, 3, 16, 16).as_subclass(Cuda)
    with pytest.raises(ValueError, match="need seg_model"):
        predict_scene(lambda t: t, x, tile=16, overlap=0, min_region=4)
    with pytest.raises(ValueError, match="need seg_model"):
        predict_scene(lambda t: t, x, tile=16, overlap=0, min_hole=4)


def test_new_names_are_exported():
    import floodgan
    from floodgan import _lib as L, model, regions, scene
    for name in ("flood_regions", "label_regions", "write_regions_csv"):
        assert name in floodgan.__all__ and getattr(floodgan, name) is getattr(regions, name)
    assert {"fg_regions_label", "fg_regions_stats", "fg_regions_table", "fg_regions_apply"} <= set(L.SIGNATURES)
    import inspect
    for fn in (scene.predict_scene, model.Model.predict_scene):
        p = inspect.signature(fn).parameters
        assert p["min_region"].default is None and p["min_hole"].default is None and p["connectivity"].default == 8
    assert regions.COLUMNS == RO.COLUMNS


def test_csv_round_trip(tmp_path):
    from floodgan.regions import write_regions_csv
    res = RO.flood_regions(RO.PATTERNS["bernoulli_0.593"](41, 53), 3, 2, 4)
    assert res["count"] > 5
    path = write_regions_csv(str(tmp_path / "regions.csv"), res)
    lines = open(path).read().split("\n")
    assert lines[0] == "label,area,y0,x0,y1,x1,sum_y,sum_x,centroid_y,centroid_x" and lines[-1] == ""
    rows = [line.split(",") for line in lines[1:-1]]
    assert len(rows) == res["count"]
    for j, name in enumerate(RO.COLUMNS):
        assert [r[j] for r in rows] == [str(v) for v in res["table"][name].tolist()], name     # integers as integers
    back = np.array([[float(r[8]), float(r[9])] for r in rows])
    assert np.array_equal(back, res["centroids"])
    with pytest.raises(ValueError, match="table=False"):
        write_regions_csv(str(tmp_path / "none.csv"), {"table": None, "centroids": None})
