"""The flood depth's semantics without a device: the two numpy oracles of the nearest-seed transform
(tests/depth_oracle.py) against each other and against scipy.ndimage, hand-checked cases, the CSV's depth columns, the
option errors and the new names."""
import numpy as np
import pytest

import depth_oracle as DO
import regions_oracle as RO

SHAPES = [(1, 1), (1, 37), (37, 1), (16, 16), (41, 53), (96, 130)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_the_separable_oracle_equals_the_brute_force_one(H, W):
    for name, make in RO.PATTERNS.items():
        for seeds in (make(H, W), ~make(H, W)):
            a, b = DO.nearest_seed_brute(seeds), DO.nearest_seed_separable(seeds)
            assert a[0].dtype == b[0].dtype == np.int32 and a[1].dtype == b[1].dtype == np.int32
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name


def test_the_oracle_equals_scipy_at_257_x_515():
    ndimage = pytest.importorskip("scipy.ndimage")
    H, W = 257, 515
    for name in ("checkerboard", "spiral", "bernoulli_0.593", "bernoulli_0.3"):
        seeds = RO.PATTERNS[name](H, W)
        near, d2 = DO.nearest_seed_separable(seeds)
        dist, ind = ndimage.distance_transform_edt(~seeds, return_indices=True)
        assert np.array_equal(np.rint(dist ** 2).astype(np.int64), d2), name
        # the index only where the minimum is unique (scipy has no tie rule): count the seeds at exactly dist2 over
        # the offsets (dy, dx) within the largest distance of the plane
        r = int(np.sqrt(d2.max()))
        assert r <= 24, (name, r)
        pad = np.zeros((H + 2 * r, W + 2 * r), dtype=bool)
        pad[r:r + H, r:r + W] = seeds
        ties = np.zeros((H, W), dtype=np.int64)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ties += pad[r + dy:r + dy + H, r + dx:r + dx + W] & (d2 == dy * dy + dx * dx)
        assert ties.min() >= 1
        unique = ties == 1
        assert unique.sum() > H * W // 4, name
        assert np.array_equal((ind[0] * W + ind[1])[unique], near[unique]), name


def test_hand_checked_ties():
    row = np.array([[1, 0, 0, 0, 1]], dtype=bool)
    for fn in (DO.nearest_seed_brute, DO.nearest_seed_separable):
        near, d2 = fn(row)
        assert near.tolist() == [[0, 0, 0, 4, 4]] and d2.tolist() == [[0, 1, 4, 1, 0]]
        corners = np.zeros((3, 3), dtype=bool)
        corners[::2, ::2] = True
        near, d2 = fn(corners)
        assert near[1, 1] == 0 and d2[1, 1] == 2
        assert near.tolist() == [[0, 0, 2], [0, 0, 2], [6, 6, 8]]
        none = fn(np.zeros((4, 5), dtype=bool))
        assert (none[0] == -1).all() and (none[1] == -1).all()


def test_a_bowl_under_a_disc_gives_the_analytic_depth():
    """elevation r^2 / 64 (exact in fp32 for integer r^2 < 2^18) under the flood disc r^2 <= 20^2: the shore is the
    disc's rim, the nearest rim pixel of p lies at r_s^2 and depth = (r_s^2 - r_p^2) / 64 exactly; at the centre every
    rim pixel with r^2 = 400 is nearest."""
    n, c = 65, 32
    yy, xx = np.mgrid[0:n, 0:n]
    r2 = (yy - c) ** 2 + (xx - c) ** 2
    mask = r2 <= 400
    elev = (r2 / 64.0).astype(np.float32)
    res = DO.flood_depth(mask, elev)
    s = DO.shore(mask)
    assert res["shore_count"] == int(s.sum()) and s[c, c + 20] and not s[c, c + 19] and not s[c, c + 21]
    near = res["nearest_shore"]
    want = (r2.ravel()[near] - r2) / 64.0
    assert np.array_equal(res["depth"][mask], want[mask].astype(np.float32)) and (res["depth"][~mask] == 0).all()
    rim = int(r2[s].min())
    assert 19 * 19 < rim <= 400 and near[c, c] == np.flatnonzero((s & (r2 == rim)).ravel())[0]
    assert res["depth"][c, c] == np.float32(rim / 64.0) and res["max_depth"] == float(res["depth"].max())
    assert (res["depth"][s] == 0).all()
    q = DO.quanta(res["depth"])
    assert res["volume"] == q.sum() / 1024.0 and res["mean_depth"] == q.sum() / 1024.0 / mask.sum()
    assert res["wet_area"] == int((mask & ~s).sum())
    # one pixel inside the row's end, the rim pixel beside it in the row and the one above are both at distance 1:
    # the one above has the smaller index
    assert s[c - 1, c + 19] and near[c, c + 19] == (c - 1) * n + c + 19 and near[c, c - 19] == (c - 1) * n + c - 19


def test_a_scene_without_a_shore_has_depth_0_and_no_nearest_pixel():
    elev = np.random.default_rng(0).random((9, 11)).astype(np.float32)
    for mask in (np.ones((9, 11), dtype=bool), np.zeros((9, 11), dtype=bool)):
        res = DO.flood_depth(mask, elev)
        assert (res["depth"] == 0).all() and (res["nearest_shore"] == -1).all()
        assert (res["shore_count"], res["max_depth"], res["mean_depth"], res["volume"]) == (0, 0.0, 0.0, 0.0)


def test_quanta_round_half_to_even_and_cap():
    d = np.array([0.0, 2.0 ** -11, 3 * 2.0 ** -11, 2.0 ** -10, 1.5, np.inf, 2.0 ** 21, -1.0], dtype=np.float32)
    assert DO.quanta(d).tolist() == [0, 0, 2, 1, 1536, 2 ** 30, 2 ** 30, -1024]


CSV_TODAY = ("label,area,y0,x0,y1,x1,sum_y,sum_x,centroid_y,centroid_x\n"
             "1,3,0,1,1,2,1,4,0.3333333333333333,1.3333333333333333\n"
             "12,2,3,0,3,1,6,1,3.0,0.5\n")


def _small_regions():
    mask = np.array([[0, 1, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0]], dtype=bool)
    return mask, RO.flood_regions(mask, 1, 0, 4)


def test_csv_without_depth_is_what_it_was_and_with_depth_reads_back(tmp_path):
    from floodgan.regions import write_regions_csv
    mask, res = _small_regions()
    path = write_regions_csv(str(tmp_path / "plain.csv"), res)
    assert open(path).read() == CSV_TODAY
    assert open(write_regions_csv(str(tmp_path / "none.csv"), res, depth=None)).read() == CSV_TODAY
    elev = np.array([[3, 1, 0.3, 2], [2, 0.1, 1, 1], [1, 1, 1, 1], [0.7, 0.2, 1.9, 1]], dtype=np.float32)
    dep = DO.flood_depth(mask, elev, res["labels"], res["table"]["area"], pixel_area=0.1)
    path = write_regions_csv(str(tmp_path / "depth.csv"), res, depth=dep)
    lines = open(path).read().split("\n")
    assert lines[0] == CSV_TODAY.split("\n")[0] + ",wet_area,mean_depth,max_depth,volume" and lines[-1] == ""
    rows = [line.split(",") for line in lines[1:-1]]
    assert [",".join(r[:10]) for r in rows] == CSV_TODAY.split("\n")[1:-1]
    assert [r[10] for r in rows] == [str(v) for v in dep["table"]["wet_area"].tolist()]
    for j, col in enumerate(("mean_depth", "max_depth", "volume")):
        back = np.array([float(r[11 + j]) for r in rows])
        assert back.dtype == np.float64 and np.array_equal(back, dep["table"][col]), col
    with pytest.raises(ValueError, match="no table of these regions"):
        write_regions_csv(str(tmp_path / "bad.csv"), res, depth={"max_depth": 0.0})


def test_option_refusals_come_before_any_launch():
    import torch

    from floodgan.depth import flood_depth, nearest_seed
    from floodgan.scene import predict_scene
    cpu = torch.zeros(4, 5)
    with pytest.raises(ValueError, match="kind must be one of"):
        nearest_seed(cpu, kind="unit")
    with pytest.raises(ValueError, match="float32 tensor on a HIP device"):
        nearest_seed(cpu)
    with pytest.raises(ValueError, match="float32 tensor on a HIP device"):
        nearest_seed(np.zeros((4, 5), np.float32))

    class Cuda(torch.Tensor):                    # passes the device checks without a device
        is_cuda = True

    with pytest.raises(ValueError, match="each side must be at most 32768"):
        nearest_seed(torch.zeros(1).expand(2, 32769).as_subclass(Cuda), kind="threshold")
    with pytest.raises(ValueError, match="the elevation is \\(4, 6\\)"):
        flood_depth(cpu, torch.zeros(4, 6))
    with pytest.raises(ValueError, match="must be \\[H, W\\] or \\[1, 1, H, W\\]"):
        flood_depth(torch.zeros(1, 3, 4, 5), cpu)
    with pytest.raises(ValueError, match="must be a float32 tensor"):
        flood_depth(cpu, torch.zeros(4, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="on one HIP device"):
        flood_depth(cpu, torch.zeros(1, 1, 4, 5))
    x = torch.zeros(1, 3, 16, 16).as_subclass(Cuda)
    with pytest.raises(ValueError, match="elevation .* needs seg_model"):
        predict_scene(lambda t: t, x, tile=16, overlap=0, elevation=torch.zeros(16, 16))
    with pytest.raises(ValueError, match="elevation must be a float32 \\[16, 16\\]"):
        predict_scene(lambda t: t, x, tile=16, overlap=0, seg_model="stub", elevation=torch.zeros(16, 17))


def test_new_names_are_exported():
    import inspect

    import floodgan
    from floodgan import _lib as L, data, depth, model, regions, scene
    for name, mod in (("nearest_seed", depth), ("flood_depth", depth), ("load_scene_elevation", data)):
        assert name in floodgan.__all__ and getattr(floodgan, name) is getattr(mod, name)
    assert {"fg_nearest_seed", "fg_nearest_seed_scratch_bytes", "fg_shore", "fg_flood_depth",
            "fg_depth_table"} <= set(L.SIGNATURES)
    p = inspect.signature(scene.predict_scene).parameters
    assert p["elevation"].default is None and p["pixel_area"].default == 1.0
    p = inspect.signature(model.Model.predict_scene).parameters
    assert p["depth"].default is False and p["pixel_area"].default == 1.0 and p["depth_vmax"].default is None
    assert inspect.signature(regions.write_regions_csv).parameters["depth"].default is None
    assert regions.DEPTH_COLUMNS == ("wet_area", "mean_depth", "max_depth", "volume")
