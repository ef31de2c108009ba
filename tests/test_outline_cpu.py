"""The region outlines' semantics without a device: the sequential tracer (tests/outline_oracle.py) held to the
identities of the ring definition and to the mask its polygons enclose, the GeoJSON writer on the tracer's results, the
argument refusals and the exports.  Everything is an integer: every comparison is exact equality."""
import functools
import inspect
import json

import numpy as np
import pytest

import outline_oracle as OO
import regions_oracle as RO

SHAPES = [(1, 1), (1, 37), (37, 1), (16, 16), (41, 53)]


def _grid(rows):
    return np.array([[c == "#" for c in r] for r in rows])


def check_identities(out, labels, table, what):
    """the three identities of the ring definition, one label per ring's start, and the order"""
    H, W = labels.shape
    r = out["rings"]
    N = out["ring_count"]
    assert N == len(r["label"]) == len(r["offset"]) - 1 and out["vertex_count"] == r["offset"][-1], what
    assert out["edge_count"] == int(r["edges"].sum()) == len(OO.crack_keys(labels >= 0)), what
    # a ring is a hole exactly when its start edge is a side 2; otherwise the start edge is a side 0
    assert np.array_equal(r["start_key"] & 3, np.where(r["hole"], 2, 0)), what
    # an outer ring starts at its region's first pixel, and every region has exactly one
    outer = ~r["hole"]
    assert np.array_equal(r["start_key"][outer], 4 * r["label"][outer]), what
    assert np.array_equal(r["label"][outer], table["label"]), what
    # the label is that of the start edge's pixel
    assert np.array_equal(labels.reshape(-1)[r["start_key"] >> 2], r["label"]), what
    # per region, area2(outer) - sum area2(holes) = 2 area
    signed = np.where(r["hole"], -r["area2"], r["area2"])
    row = np.searchsorted(table["label"], r["label"])
    assert np.array_equal(np.bincount(row, weights=signed, minlength=len(table["label"])).astype(np.int64),
                          2 * table["area"]), what
    # ascending (label, start_key)
    order = np.lexsort((r["start_key"], r["label"]))
    assert np.array_equal(order, np.arange(N)), what
    # every ring has at least four corners, and no two consecutive ones coincide
    assert (np.diff(r["offset"]) >= 4).all(), what


@functools.lru_cache(maxsize=None)
def _case(H, W, name, connectivity):
    labels = RO.label(RO.PATTERNS[name](H, W), connectivity)
    return labels, RO.table(labels), OO.outlines(labels, connectivity)


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("H,W", SHAPES)
def test_the_tracer_satisfies_the_identities_and_encloses_the_mask(H, W, connectivity):
    for name in RO.PATTERNS:
        labels, table, out = _case(H, W, name, connectivity)
        what = (name, H, W, connectivity)
        check_identities(out, labels, table, what)
        assert np.array_equal(OO.rebuild_mask(out, H, W), labels >= 0), what


@pytest.mark.parametrize("connectivity", [8, 4])
def test_one_label_on_the_left_of_every_ring(connectivity):
    """walked on the vertices: every unit step of a ring has a flood pixel of the ring's label on its left"""
    left = {(0, -1): (0, -1), (1, 0): (0, 0), (0, 1): (-1, 0), (-1, 0): (-1, -1)}   # step -> pixel - start vertex
    for H, W in SHAPES:
        for name in RO.PATTERNS:
            labels, _, out = _case(H, W, name, connectivity)
            r, steps = out["rings"], 0
            for k in range(out["ring_count"]):
                v = out["vertices"][r["offset"][k]:r["offset"][k + 1]].astype(np.int64)
                for (y0, x0), (y1, x1) in zip(v.tolist(), np.roll(v, -1, axis=0).tolist()):
                    assert (y0 == y1) != (x0 == x1)                               # axis-parallel and not empty
                    n = abs(y1 - y0) + abs(x1 - x0)
                    dy, dx = (y1 - y0) // n, (x1 - x0) // n
                    py, px = left[(dy, dx)]
                    for t in range(n):
                        assert labels[y0 + t * dy + py, x0 + t * dx + px] == r["label"][k], (name, H, W, k)
                    steps += n
            assert steps == out["edge_count"], (name, H, W)


def test_hand_checked_rings():
    # one pixel: the four sides, counter-clockwise in a north-up picture, from the start edge's start vertex
    out = OO.outlines(RO.label(_grid(["#"]), 8), 8)
    assert out["vertices"].tolist() == [[0, 1], [0, 0], [1, 0], [1, 1]]
    assert (out["edge_count"], out["ring_count"], out["rings"]["area2"].tolist()) == (4, 1, [2])
    # a row: the start edge's start vertex (0, 1) is no corner, so the list begins at the next one
    out = OO.outlines(RO.label(_grid(["###"]), 8), 8)
    assert out["vertices"].tolist() == [[0, 0], [1, 0], [1, 3], [0, 3]] and out["rings"]["edges"].tolist() == [8]
    # a frame: the outer ring, then its hole, clockwise, from the hole's top-left corner
    out = OO.outlines(RO.label(_grid(["###", "#.#", "###"]), 8), 8)
    assert out["rings"]["hole"].tolist() == [False, True] and out["rings"]["area2"].tolist() == [18, 2]
    assert out["rings"]["start_key"].tolist() == [0, 4 * 1 + 2]
    assert out["vertices"][4:].tolist() == [[1, 1], [1, 2], [2, 2], [2, 1]]
    # a saddle: one ring through the shared vertex twice at 8, two rings at 4
    m = _grid(["#.", ".#"])
    out = OO.outlines(RO.label(m, 8), 8)
    assert out["ring_count"] == 1 and out["rings"]["edges"].tolist() == [8]
    assert out["vertices"].tolist() == [[0, 1], [0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1]]
    out = OO.outlines(RO.label(m, 4), 4)
    assert out["ring_count"] == 2 and out["rings"]["label"].tolist() == [0, 3]
    # a dry saddle inside a region: one hole at 4 (the dry class is 8-connected), two at 8
    m = _grid(["####", "#.##", "##.#", "####"])
    assert OO.outlines(RO.label(m, 4), 4)["rings"]["hole"].tolist() == [False, True]
    assert OO.outlines(RO.label(m, 8), 8)["rings"]["hole"].tolist() == [False, True, True]
    # nothing floods
    out = OO.outlines(RO.label(_grid(["..", ".."]), 8), 8)
    assert (out["edge_count"], out["ring_count"], out["vertex_count"]) == (0, 0, 0)
    assert out["vertices"].shape == (0, 2) and out["rings"]["offset"].tolist() == [0]


def test_the_long_rings_of_the_issue():
    for name, H, W, edges in [("spiral", 41, 53, 2268), ("serpentine", 41, 53, 2268), ("spiral", 96, 130, 12672),
                              ("serpentine", 96, 130, 12576)]:
        out = OO.outlines(RO.label(RO.PATTERNS[name](H, W), 8), 8)
        assert out["rings"]["edges"].tolist() == [edges], (name, H, W)


def _regions_and_depth(H=41, W=53, name="frame_island", connectivity=8):
    res = RO.flood_regions(RO.PATTERNS[name](H, W), 1, 0, connectivity)
    R = res["count"]
    rng = np.random.default_rng(3)
    depth = {"table": {"wet_area": np.arange(R, dtype=np.int64) + 5, "mean_depth": rng.random(R),
                       "max_depth": rng.random(R) + 1, "volume": rng.random(R) * 100}}
    return res, OO.outlines(res["labels"], connectivity), depth


def test_geojson_structure_and_determinism(tmp_path):
    from floodgan.outline import write_regions_geojson
    for name, connectivity in [("frame_island", 8), ("bernoulli_0.593", 4), ("checkerboard", 8), ("dry", 8)]:
        res, out, depth = _regions_and_depth(name=name, connectivity=connectivity)
        path = str(tmp_path / f"{name}.geojson")
        assert write_regions_geojson(path, res, out) == path
        first = open(path, "rb").read()
        doc = json.loads(first)
        assert list(doc) == ["type", "features"] and doc["type"] == "FeatureCollection"
        assert len(doc["features"]) == res["count"]
        r = out["rings"]
        for row, feat in enumerate(doc["features"]):
            assert list(feat) == ["type", "properties", "geometry"] and feat["type"] == "Feature"
            assert feat["geometry"]["type"] == "Polygon"
            p = feat["properties"]
            assert list(p) == ["label", "area", "y0", "x0", "y1", "x1", "centroid_y", "centroid_x", "perimeter", "holes"]
            for col in ("label", "area", "y0", "x0", "y1", "x1"):
                assert p[col] == res["table"][col][row] and isinstance(p[col], int)
            assert p["centroid_y"] == res["centroids"][row, 0] and p["centroid_x"] == res["centroids"][row, 1]
            mine = np.flatnonzero(r["label"] == p["label"])
            assert p["perimeter"] == r["edges"][mine].sum() and p["holes"] == len(mine) - 1 == r["hole"][mine].sum()
            rings = feat["geometry"]["coordinates"]
            assert len(rings) == len(mine)
            for k, ring in zip(mine, rings):
                v = out["vertices"][r["offset"][k]:r["offset"][k + 1]]
                assert ring[0] == ring[-1] and len(ring) == len(v) + 1                   # closed
                assert all(isinstance(c, int) for pt in ring for c in pt)
                assert ring[:-1] == [[int(x), int(y)] for y, x in v]                    # [x, y]
            # outer first: counter-clockwise with y up (negative shoelace sum with y down), then the holes
            for k, ring in enumerate(rings):
                s = sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring, ring[1:]))
                assert (s < 0) == (k == 0)
        assert write_regions_geojson(str(tmp_path / "again.geojson"), res, out) and \
            open(str(tmp_path / "again.geojson"), "rb").read() == first
    assert json.loads(first) == {"type": "FeatureCollection", "features": []}                # the dry scene


def test_geojson_transform_and_depth_columns(tmp_path):
    from floodgan.outline import write_regions_geojson
    res, out, depth = _regions_and_depth()
    t = (300000.25, 10.0, 0.125, 4100000.5, -0.375, -10.0)
    plain = json.load(open(write_regions_geojson(str(tmp_path / "a.geojson"), res, out)))
    moved = json.load(open(write_regions_geojson(str(tmp_path / "b.geojson"), res, out, depth, t)))
    assert res["count"] == 2 and [f["properties"]["holes"] for f in plain["features"]] == [1, 0]
    for row, (fa, fb) in enumerate(zip(plain["features"], moved["features"])):
        for ra, rb in zip(fa["geometry"]["coordinates"], fb["geometry"]["coordinates"]):
            want = [[t[0] + float(x) * t[1] + float(y) * t[2], t[3] + float(x) * t[4] + float(y) * t[5]] for x, y in ra]
            assert rb == want and all(isinstance(c, float) for pt in rb for c in pt)
        pa, pb = fa["properties"], fb["properties"]
        assert list(pb) == list(pa) + ["wet_area", "mean_depth", "max_depth", "volume"]
        assert "wet_area" not in pa and {k: pb[k] for k in pa} == pa
        assert pb["wet_area"] == depth["table"]["wet_area"][row] and isinstance(pb["wet_area"], int)
        for col in ("mean_depth", "max_depth", "volume"):
            assert pb[col] == depth["table"][col][row]                                      # repr round-trips fp64


def test_geojson_refusals(tmp_path):
    from floodgan.outline import write_regions_geojson
    res, out, depth = _regions_and_depth()
    path = str(tmp_path / "x.geojson")
    with pytest.raises(ValueError, match="table=False"):
        write_regions_geojson(path, dict(res, table=None, centroids=None), out)
    _, other, _ = _regions_and_depth(name="bernoulli_0.5")
    with pytest.raises(ValueError, match="outer rings are not the regions"):
        write_regions_geojson(path, res, other)
    with pytest.raises(ValueError, match="no table of these regions"):
        write_regions_geojson(path, res, out, {"table": None})
    with pytest.raises(ValueError, match="6-tuple"):
        write_regions_geojson(path, res, out, None, (1.0, 2.0))


def test_argument_refusals_come_before_any_launch():
    import torch

    from floodgan.outline import region_outlines
    from floodgan.scene import predict_scene

    class Cuda(torch.Tensor):                    # passes for a device tensor without a device
        is_cuda = True

    ok = torch.zeros((4, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="connectivity must be 4 or 8 \\(got 6\\)"):
        region_outlines(ok.as_subclass(Cuda), 6)
    with pytest.raises(ValueError, match="must be an int32 tensor"):
        region_outlines(torch.zeros((4, 4), dtype=torch.int64).as_subclass(Cuda))
    with pytest.raises(ValueError, match="must be an int32 tensor"):
        region_outlines(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="plane on a HIP device"):
        region_outlines(ok)
    with pytest.raises(ValueError, match="plane on a HIP device"):
        region_outlines(torch.zeros((1, 4, 4), dtype=torch.int32).as_subclass(Cuda))
    with pytest.raises(ValueError, match="below 2\\^29"):
        region_outlines(torch.zeros(1, dtype=torch.int32).expand(32768, 16384).as_subclass(Cuda))
    x = torch.zeros(1, 3, 16, 16).as_subclass(Cuda)
    with pytest.raises(ValueError, match="needs seg_model"):
        predict_scene(lambda t: t, x, tile=16, overlap=0, polygons=True)


def test_new_names_are_exported():
    import floodgan
    from floodgan import _lib as L, model, outline, scene
    for name in ("region_outlines", "write_regions_geojson"):
        assert name in floodgan.__all__ and getattr(floodgan, name) is getattr(outline, name)
    assert {"fg_outline_scratch_bytes", "fg_outline_launches", "fg_outline_cracks", "fg_outline_rings",
            "fg_outline_vertices"} <= set(L.SIGNATURES)
    for fn in (scene.predict_scene, model.Model.predict_scene):
        assert inspect.signature(fn).parameters["polygons"].default is False
    assert inspect.signature(model.Model.predict_scene).parameters["transform"].default is None
    lib = L.load()
    assert lib.fg_outline_scratch_bytes(0) == 0 and lib.fg_outline_scratch_bytes(5) == 8 * 5 + 8 * 24
    assert [lib.fg_outline_launches(E) for E in (0, 1, 4, 5, 2268, 4096)] == [1, 4, 8, 10, 28, 28]
