"""The region outlines on the HIP path (csrc/outline.hip through floodgan.outline) against the sequential tracer
(tests/outline_oracle.py), against the region table of flood_regions and against the mask their polygons enclose.
Everything is an integer: every comparison is exact equality.

A workgroup is 256 lanes and a ring is ordered by ceil(log2 E) doubling rounds: the spiral and the serpentine are
single rings of 2 268 edges at 41 x 53 and of 12 672 and 12 576 at 96 x 130 -- longer than a workgroup and no powers
of two --, the checkerboard at 8 is one ring through every saddle around about H W / 2 four-edge holes, `dry` has no
edge at all."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import outline_oracle as OO
import regions_oracle as RO
from test_outline_cpu import check_identities
from tiff_util import write_tiff

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 1), (1, 37), (37, 1), (16, 16), (41, 53), (96, 130)]
BIG = (257, 515)
BIG_PATTERNS = ["flood", "checkerboard", "spiral", "serpentine", "bernoulli_0.593"]
CASES = [(H, W, name) for H, W in SHAPES for name in RO.PATTERNS] + [BIG + (name,) for name in BIG_PATTERNS]
RING_DTYPES = {"label": np.int64, "start_key": np.int64, "edges": np.int64, "area2": np.int64, "hole": np.bool_,
               "offset": np.int64}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from floodgan import _lib as L
    L.load()


@functools.lru_cache(maxsize=None)
def _mask(H, W, name):
    m = RO.PATTERNS[name](H, W)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _oracle(H, W, name, connectivity):
    """(labels, outlines) of the numpy oracles; computed once per module, read-only"""
    labels = RO.label(_mask(H, W, name), connectivity)
    labels.setflags(write=False)
    return labels, OO.outlines(labels, connectivity)


def _plane(mask):
    return torch.from_numpy(mask.astype(np.float32))[None, None].to(DEV)


def _shape_cases(H, W):
    return [name for h, w, name in CASES if (h, w) == (H, W)]


def _same_outlines(got, want, what):
    assert set(got) == {"edge_count", "ring_count", "vertex_count", "rings", "vertices"}, what
    for key in ("edge_count", "ring_count", "vertex_count"):
        assert got[key] == want[key] and isinstance(got[key], int), (what, key)
    assert set(got["rings"]) == set(RING_DTYPES), what
    for col, dtype in RING_DTYPES.items():
        assert got["rings"][col].dtype == dtype and np.array_equal(got["rings"][col], want["rings"][col]), (what, col)
    assert got["vertices"].dtype == np.int32 and got["vertices"].shape == (want["vertex_count"], 2), what
    assert np.array_equal(got["vertices"], want["vertices"]), what


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("H,W", SHAPES + [BIG])
def test_region_outlines_equal_the_oracle(H, W, connectivity):
    from floodgan.outline import region_outlines
    from floodgan.regions import label_regions
    for name in _shape_cases(H, W):
        labels, want = _oracle(H, W, name, connectivity)
        dev = label_regions(_plane(_mask(H, W, name)), "threshold", True, connectivity)
        assert np.array_equal(dev.cpu().numpy(), labels), name
        _same_outlines(region_outlines(dev, connectivity), want, (name, H, W, connectivity))
    # the cases the shapes are there for
    if (H, W) in ((41, 53), (96, 130)):
        edges = {(41, 53): (2268, 2268), (96, 130): (12672, 12576)}[(H, W)]
        for name, n in zip(("spiral", "serpentine"), edges):
            assert _oracle(H, W, name, connectivity)[1]["rings"]["edges"].tolist() == [n]
    if (H, W) == (96, 130) and connectivity == 8:
        cb = _oracle(H, W, "checkerboard", 8)[1]
        inner_dry = int((~_mask(H, W, "checkerboard"))[1:-1, 1:-1].sum())
        assert cb["ring_count"] == 1 + inner_dry == 1 + (H - 2) * (W - 2) // 2
        assert (cb["rings"]["edges"][1:] == 4).all() and cb["rings"]["hole"][1:].all()
    assert _oracle(H, W, "flood", connectivity)[1]["edge_count"] == 2 * (H + W)
    if (H, W) != BIG:
        assert _oracle(H, W, "dry", connectivity)[1]["edge_count"] == 0


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("H,W", [(41, 53), (96, 130), BIG])
def test_area_identity_and_rebuilt_mask_without_the_tracer(H, W, connectivity):
    """the device result against flood_regions' own table and against the mask: no oracle tracer involved"""
    from floodgan.outline import region_outlines
    from floodgan.regions import flood_regions
    for name in _shape_cases(H, W):
        reg = flood_regions(_plane(_mask(H, W, name)), "threshold", 1, 0, connectivity)
        out = region_outlines(reg["labels"], connectivity)
        what = (name, H, W, connectivity)
        if reg["count"] == 0:
            assert out["edge_count"] == 0 and out["ring_count"] == 0, what
            continue
        check_identities(out, reg["labels"].cpu().numpy(), reg["table"], what)
        assert np.array_equal(OO.rebuild_mask(out, H, W), _mask(H, W, name)), what


def test_sieved_regions_and_the_other_connectivity():
    """the outlines follow the labels plane they are given: a sieved one, and one traced at the connectivity its
    labels were not made with (rings then mix labels, but the polygons still enclose the mask)"""
    from floodgan.outline import region_outlines
    from floodgan.regions import flood_regions
    H, W, name = 96, 130, "bernoulli_0.593"
    reg = flood_regions(_plane(_mask(H, W, name)), "threshold", 8, 8, 4)
    labels = reg["labels"].cpu().numpy()
    _same_outlines(region_outlines(reg["labels"], 4), OO.outlines(labels, 4), "sieved")
    other = region_outlines(reg["labels"], 8)
    _same_outlines(other, OO.outlines(labels, 8), "other connectivity")
    assert np.array_equal(OO.rebuild_mask(other, H, W), labels >= 0)


def test_two_calls_are_bit_identical():
    from floodgan.outline import region_outlines
    from floodgan.regions import label_regions
    for name, connectivity in [("bernoulli_0.593", 4), ("checkerboard", 8), ("spiral", 8)]:
        labels = label_regions(_plane(_mask(96, 130, name)), "threshold", True, connectivity)
        a, b = (region_outlines(labels, connectivity) for _ in range(2))
        for col in RING_DTYPES:
            assert a["rings"][col].tobytes() == b["rings"][col].tobytes(), (name, col)
        assert a["vertices"].tobytes() == b["vertices"].tobytes(), name


def test_refused_calls_leave_their_outputs_as_they_were():
    import ctypes as C

    from floodgan import _lib as L, ops
    from floodgan.outline import region_outlines
    from floodgan.regions import label_regions
    lib = L.load()
    H, W = 16, 16
    labels = label_regions(_plane(_mask(H, W, "frame_island")), "threshold", True, 8)
    want = _oracle(H, W, "frame_island", 8)[1]
    E, V = want["edge_count"], want["vertex_count"]
    sides = torch.full((H, W), 77, dtype=torch.uint8, device=DEV)
    count = torch.full((H, W), 77, dtype=torch.int32, device=DEV)
    incl = torch.full((H * W,), 77, dtype=torch.int32, device=DEV)
    out = {name: torch.full((E,), 77, dtype=torch.int32, device=DEV) for name in ("key", "ring", "edges", "corners")}
    out["signed2"] = torch.full((E,), 77, dtype=torch.int64, device=DEV)
    out["corner"] = torch.full((E,), 77, dtype=torch.uint8, device=DEV)
    base = torch.full((E,), 77, dtype=torch.int32, device=DEV)
    vertices = torch.full((V, 2), 77, dtype=torch.int32, device=DEV)
    nbytes = lib.fg_outline_scratch_bytes(E)
    assert nbytes == 8 * E + 8 * ((4 * E + 7) // 8 * 8) and lib.fg_outline_scratch_bytes(-1) == 0
    scratch = torch.full((nbytes // 8,), 77, dtype=torch.int64, device=DEV)
    st, null, p = L.stream_handle(), C.c_void_p(0), L.ptr
    odd = lambda t: C.c_void_p(t.data_ptr() + 2)                                  # noqa: E731

    def rings(labels_=p(labels), sides_=p(sides), incl_=p(incl), H_=H, W_=W, conn=8, E_=E, key=p(out["key"]),
              ring=p(out["ring"]), signed2=p(out["signed2"]), corner=p(out["corner"]), scratch_=p(scratch)):
        return lib.fg_outline_rings(labels_, sides_, incl_, H_, W_, conn, E_, key, ring, p(out["edges"]),
                                    p(out["corners"]), signed2, corner, scratch_, st)

    def verts(key=p(out["key"]), base_=p(base), H_=H, E_=E, V_=V, vertices_=p(vertices)):
        return lib.fg_outline_vertices(key, p(out["ring"]), p(out["corners"]), p(out["corner"]), base_, H_, W, E_, V_,
                                       vertices_, st)

    refused = [
        lib.fg_outline_cracks(null, H, W, p(sides), p(count), st),
        lib.fg_outline_cracks(p(labels), H, W, null, p(count), st),
        lib.fg_outline_cracks(p(labels), H, W, p(sides), null, st),
        lib.fg_outline_cracks(p(labels), 0, W, p(sides), p(count), st),
        lib.fg_outline_cracks(p(labels), 32768, 16384, p(sides), p(count), st),      # H W = 2^29
        lib.fg_outline_cracks(p(labels), H, W, p(sides), odd(count), st),
        rings(labels_=null), rings(sides_=null), rings(incl_=null), rings(key=null), rings(corner=null),
        rings(scratch_=null), rings(H_=0), rings(H_=32768, W_=16384), rings(conn=6), rings(E_=0),
        rings(E_=4 * H * W + 1), rings(ring=odd(out["ring"])),
        rings(signed2=C.c_void_p(out["signed2"].data_ptr() + 4)), rings(scratch_=C.c_void_p(scratch.data_ptr() + 4)),
        verts(key=null), verts(base_=null), verts(vertices_=null), verts(H_=0), verts(E_=0), verts(V_=0),
        verts(V_=E + 1), verts(vertices_=odd(vertices)),
    ]
    assert refused == [-1] * len(refused)                     # FG_ERR_INVALID
    assert b"fg_outline_vertices" in lib.fg_last_error()
    # the Python wrappers, before the library is called
    with pytest.raises(RuntimeError, match="side plane is a contiguous"):
        ops.outline_cracks(labels, torch.full((H, W), 77, dtype=torch.int32, device=DEV), count)
    with pytest.raises(RuntimeError, match="the ring array is a contiguous"):
        ops.outline_rings(labels, sides, incl, 8, dict(out, ring=torch.full((E + 1,), 77, dtype=torch.int32,
                                                                            device=DEV)))
    with pytest.raises(ValueError, match="below 2\\^29"):
        region_outlines(torch.zeros(1, dtype=torch.int32, device=DEV).expand(32768, 16384))
    with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
        region_outlines(labels, 6)
    with pytest.raises(ValueError, match="int32 tensor"):
        region_outlines(labels.long())
    torch.cuda.synchronize()
    for t in [sides, count, incl, base, vertices, scratch] + list(out.values()):
        assert bool((t == 77).all())
    # and the same buffers take the accepted calls
    ops.outline_cracks(labels, sides, count)
    incl = torch.cumsum(count.view(-1), 0, dtype=torch.int32)
    assert int(incl[-1]) == E
    ops.outline_rings(labels, sides, incl, 8, out)
    starts = torch.nonzero(out["ring"] == torch.arange(E, dtype=torch.int32, device=DEV)).view(-1)
    assert np.array_equal(np.sort(out["key"][starts].cpu().numpy()), np.sort(want["rings"]["start_key"]))
    assert np.array_equal(np.sort(out["edges"][starts].cpu().numpy()), np.sort(want["rings"]["edges"]))
    assert int(out["corners"][starts].sum()) == V and int(out["corner"].sum()) == V


class _Identity(torch.nn.Module):
    def forward(self, x):
        return x[:, :3]


def _patch_unet(monkeypatch):
    """predict_scene's U-Net path replaced by a known logit pattern: +4 where the picture's first channel is positive,
    -4 elsewhere (as tests/test_gpu_regions.py does: blended, such a logit keeps its sign)"""
    from floodgan import scene
    monkeypatch.setattr(scene, "_unet", lambda seg_model, batch_stats: seg_model)
    monkeypatch.setattr(scene, "_flood_logits",
                        lambda unet, images, batch_stats: torch.where(images[:, :1] > 0, 4.0, -4.0))


def test_predict_scene_gains_the_outlines_only_when_asked(monkeypatch):
    from floodgan.scene import predict_scene
    _patch_unet(monkeypatch)
    H, W, tile, overlap = 48, 56, 16, 8
    mask = RO.bernoulli(H, W, 0.593, 593)
    x = torch.from_numpy(np.where(mask, 0.5, -0.5).astype(np.float32))[None, None].repeat(1, 3, 1, 1).to(DEV)
    plain = predict_scene(_Identity(), x, tile=tile, overlap=overlap, batch=5, seg_model="stub")
    assert set(plain) == {"grid", "output", "flood_logits", "flood_fraction"}                 # today's keys, exactly
    sieved = predict_scene(_Identity(), x, tile=tile, overlap=overlap, batch=5, seg_model="stub", min_region=8)
    assert set(sieved) == set(plain) | {"flood_mask", "regions", "flood_fraction_sieved"}     # and today's with minima
    for min_region, min_hole, connectivity in [(None, None, 8), (None, None, 4), (8, 8, 4)]:
        res = predict_scene(_Identity(), x, tile=tile, overlap=overlap, batch=5, seg_model="stub",
                            min_region=min_region, min_hole=min_hole, connectivity=connectivity, polygons=True)
        extra = {"flood_mask", "regions", "outlines"} | ({"flood_fraction_sieved"} if min_region else set())
        assert set(res) == set(plain) | extra
        assert torch.equal(res["flood_logits"], plain["flood_logits"]) and torch.equal(res["output"], plain["output"])
        want = RO.flood_regions(mask, min_region or 1, min_hole or 0, connectivity)
        assert np.array_equal(res["regions"]["labels"].cpu().numpy(), want["labels"])
        _same_outlines(res["outlines"], OO.outlines(want["labels"], connectivity), (min_region, connectivity))
    with pytest.raises(ValueError, match="needs seg_model"):
        predict_scene(_Identity(), x, tile=tile, overlap=overlap, polygons=True)
    with pytest.raises(ValueError, match="connectivity 6"):
        predict_scene(_Identity(), x, tile=tile, overlap=overlap, seg_model="stub", polygons=True, connectivity=6)


def test_model_predict_scene_writes_the_geojson_beside_the_csv(tmp_path, monkeypatch):
    from floodgan.model import Model
    _patch_unet(monkeypatch)
    root = str(tmp_path)
    H, W = 40, 56
    raw = np.random.default_rng(21).random((H, W, 9)).astype(np.float32)
    path = os.path.join(root, "harvey_scene.tif")
    write_tiff(path, raw)
    m = Model(model="PairedAttention", training_model=False, data_path=root, resize=None, crop=None,
              train_loader=[], device=DEV)
    kw = dict(tile=32, overlap=8, batch=3, seg_model_path="stub")
    before = m.predict_scene(path, **kw)
    assert set(before) == {"prediction", "flood_mask", "flood_fraction", "grid"}              # today's keys, exactly
    assert sorted(os.listdir(f"{root}/images")) == ["harvey_scene_floodMask.png", "harvey_scene_prediction.png"]
    sieved = m.predict_scene(path, min_region=6, min_hole=6, connectivity=4, **kw)
    assert set(sieved) == set(before) | {"regions", "region_count"}
    files = {f: open(f"{root}/images/{f}", "rb").read() for f in os.listdir(f"{root}/images")}
    assert sorted(files) == ["harvey_scene_floodMask.png", "harvey_scene_floodRegions.csv",
                             "harvey_scene_prediction.png"]
    with pytest.raises(ValueError, match="needs seg_model_path"):
        m.predict_scene(path, tile=32, overlap=8, polygons=True)
    t = (500000.0, 30.0, 0.0, 3300000.0, 0.0, -30.0)
    for depth, transform in [(False, None), (True, t)]:
        written = m.predict_scene(path, min_region=6, min_hole=6, connectivity=4, polygons=True, depth=depth,
                                  transform=transform, **kw)
        assert written["polygons"] == f"{root}/images/harvey_scene_floodRegions.geojson"
        assert set(written) == set(sieved) | {"polygons"} | ({"flood_depth", "max_depth", "mean_depth", "volume"}
                                                             if depth else set())
        if not depth:                                       # the other files are what they are without the polygons
            for f, data in files.items():
                assert open(f"{root}/images/{f}", "rb").read() == data, f
        doc = json.load(open(written["polygons"]))
        lines = open(written["regions"]).read().splitlines()
        head, rows = lines[0].split(","), [line.split(",") for line in lines[1:]]
        assert len(doc["features"]) == len(rows) == written["region_count"] > 3
        out = m.last_scene["outlines"]
        r = out["rings"]
        logits = m.last_scene["flood_logits"][0, 0].cpu().numpy()
        want = RO.flood_regions(logits > 0, 6, 6, 4)
        _same_outlines(out, OO.outlines(want["labels"], 4), "model")
        for feat, row in zip(doc["features"], rows):
            p = feat["properties"]
            csv = dict(zip(head, row))
            shared = [c for c in head if c in p]
            assert shared == [c for c in head if c not in ("sum_y", "sum_x")] and len(shared) == (12 if depth else 8)
            for c in shared:                                 # integers as integers, floats by repr, as the CSV has them
                assert (str(p[c]) if isinstance(p[c], int) else repr(p[c])) == csv[c], c
            mine = np.flatnonzero(r["label"] == p["label"])
            assert p["perimeter"] == r["edges"][mine].sum() and p["holes"] == len(mine) - 1
            for k, ring in zip(mine, feat["geometry"]["coordinates"]):
                v = out["vertices"][r["offset"][k]:r["offset"][k + 1]].astype(np.float64)
                pts = [[int(x), int(y)] for y, x in v] if transform is None else \
                    [[t[0] + x * t[1] + y * t[2], t[3] + x * t[4] + y * t[5]] for y, x in v]
                assert ring == pts + pts[:1]
