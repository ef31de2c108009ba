"""The flow routing on the HIP path (csrc/flow.hip through floodgan.flow) against the numpy oracle
(tests/flow_oracle.py).  Directions are decided by an exact fp64 key, everything after them is integers: every
comparison is exact equality, dtypes included.

Shapes.  The kernels run one lane per pixel in blocks of 256 with whole-wave loop bounds: 1 x 1 is one lane, 1 x 37 and
37 x 1 are a partial wave with a one-pixel axis (no north / south or no east / west neighbour anywhere), 16 x 16 one
block, 41 x 53 nine blocks with a partial last one and no side a multiple of anything, 96 x 130 the shape of the
conditions (tests/test_flow_cpu.py), and 257 x 515 a spiral path of more than 2^16 steps, which needs every one of its
18 doubling rounds.  K = 1, 6, 6, 8, 12, 14, 18: odd and even, so the chain starts in the caller's arrays and in the
scratch."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import flow_oracle as FO
import regions_oracle as RO
import render_oracle as PO
from tiff_util import write_tiff

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 1), (1, 37), (37, 1), (16, 16), (41, 53), (96, 130)]
BIG = (257, 515)
BIG_PATTERNS = ["cone", "spiral", "serpentine", "terraces", "noise"]
ROUNDS = (0, 3, 64)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from floodgan import _lib as L
    L.load()


@functools.lru_cache(maxsize=None)
def _elev(name, H, W):
    z = FO.PATTERNS[name](H, W)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _oracle(name, H, W, R):
    res = FO.flow(_elev(name, H, W), R)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                # (a copy: the cached planes are read-only)


def _same_directions(got, want, what):
    assert got["directions"].dtype == torch.uint8 and got["directions"].is_cuda, what
    assert tuple(got["directions"].shape) == want["directions"].shape, what
    assert np.array_equal(got["directions"].cpu().numpy(), want["directions"]), what
    assert got["flat_directed"].dtype == np.int32 and got["flat_directed"].shape == want["flat_directed"].shape, what
    assert np.array_equal(got["flat_directed"], want["flat_directed"]), what
    for key in ("pit_count", "nodata_count"):
        assert got[key] == want[key] and type(got[key]) is int, (what, key)


def _same_flow(got, want, what):
    _same_directions(got, want, what)
    for key in ("accumulation", "basin", "length"):
        assert got[key].dtype == torch.int32 and got[key].is_cuda, (what, key)
        assert tuple(got[key].shape) == want[key].shape, (what, key)
        assert np.array_equal(got[key].cpu().numpy(), want[key]), (what, key)
    assert got["rounds"] == want["rounds"] and type(got["rounds"]) is int, what
    assert set(got) == set(want), what


def _check(name, H, W):
    from floodgan.flow import flow_accumulation, flow_directions
    elev = _dev(_elev(name, H, W))
    for R in ROUNDS:
        want = _oracle(name, H, W, R)
        _same_flow(flow_accumulation(elev, flat_rounds=R), want, (name, H, W, R))
        got = flow_directions(elev, R)
        assert set(got) == {"directions", "pit_count", "nodata_count", "flat_directed"}
        _same_directions(got, want, (name, H, W, R, "directions alone"))
    assert want["rounds"] == FO.rounds(H, W)


@pytest.mark.parametrize("H,W", SHAPES)
def test_flow_equals_the_oracle(H, W):
    for name in FO.PATTERNS:
        _check(name, H, W)


@pytest.mark.parametrize("name", BIG_PATTERNS)
def test_flow_equals_the_oracle_at_257_x_515(name):
    _check(name, *BIG)
    if name == "spiral":
        assert _oracle(name, *BIG, 0)["length"].max() >= 2 ** 16 and _oracle(name, *BIG, 0)["rounds"] == 18


def test_a_direction_plane_gives_what_its_elevation_gives():
    from floodgan.flow import flow_accumulation
    for name, H, W, R in (("terraces", 96, 130, 64), ("holes", 41, 53, 0), ("spiral", 96, 130, 0)):
        want = _oracle(name, H, W, R)
        from_elev = flow_accumulation(_dev(_elev(name, H, W)), flat_rounds=R)
        for plane in (from_elev["directions"], _dev(want["directions"])[None, None]):
            got = flow_accumulation(directions=plane)
            for key in ("directions", "accumulation", "basin", "length"):
                assert torch.equal(got[key], from_elev[key]), (name, key)
            assert (got["pit_count"], got["nodata_count"], got["rounds"]) == \
                (want["pit_count"], want["nodata_count"], want["rounds"])
            assert got["flat_directed"].shape == (0,) and got["flat_directed"].dtype == np.int32


def test_invalid_bytes_and_pointers_out_of_the_scene_are_pits():
    """Read-side validation: a byte that is no code, a direction that leaves the scene and one that names a nodata
    pixel make a pit.  Turning pixels into pits cannot close a cycle, so the oracle's peeling still applies."""
    from floodgan.flow import flow_accumulation
    H, W = 41, 53
    d = _oracle("noise", H, W, 0)["directions"].copy()
    rng = np.random.default_rng(9)
    bad = rng.random((H, W)) < 0.05
    d[bad] = rng.integers(9, 255, int(bad.sum())).astype(np.uint8)                  # 9 .. 254: no code
    d[0, ::3], d[H - 1, ::4], d[::5, 0], d[::2, W - 1] = 6, 2, 4, 0                 # N, S, W, E out of the scene
    d[0, 0], d[0, W - 1], d[H - 1, 0], d[H - 1, W - 1] = 5, 7, 3, 1                 # the corners, diagonally out
    d[H // 2, 3:W - 3:6] = FO.NODATA                                                # nodata that neighbours point at
    recv = FO.receivers(d)
    named = d.ravel() < 8
    assert (named & (recv < 0)).sum() > 60 and (d.ravel()[recv[recv >= 0]] != FO.NODATA).all()
    acc, basin, length = FO.accumulate(d)
    got = flow_accumulation(directions=_dev(d))
    for key, want in (("accumulation", acc), ("basin", basin), ("length", length)):
        assert np.array_equal(got[key].cpu().numpy(), want), key
    pits = np.flatnonzero(recv < 0)
    pits = pits[d.ravel()[pits] != FO.NODATA]
    assert np.array_equal(basin.ravel()[pits], pits) and int(acc.ravel()[pits].sum()) == int((d != FO.NODATA).sum())
    assert got["pit_count"] == int((d == FO.PIT).sum())                             # the count is of the byte 8


def test_two_calls_are_bit_identical():
    from floodgan.flow import flow_accumulation
    for name in ("cone", "noise"):                  # one confluence of the whole scene, and thousands of small ones
        elev = _dev(_elev(name, *BIG))
        a, b = flow_accumulation(elev, flat_rounds=3), flow_accumulation(elev, flat_rounds=3)
        for key in ("directions", "accumulation", "basin", "length"):
            assert torch.equal(a[key], b[key]), (name, key)
        assert np.array_equal(a["flat_directed"], b["flat_directed"])


def test_a_four_dimensional_view_and_another_stream():
    from floodgan.flow import flow_accumulation
    name, H, W, R = "terraces", 96, 130, 3
    want = _oracle(name, H, W, R)
    elev = _dev(_elev(name, H, W))
    _same_flow(flow_accumulation(elev[None, None], flat_rounds=R), want, "[1, 1, H, W]")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = flow_accumulation(elev, flat_rounds=R)
    stream.synchronize()
    _same_flow(got, want, "stream")


def test_refused_calls_leave_their_outputs_as_they_were():
    from floodgan import _lib as L, flow, ops
    lib = L.load()
    H, W = 16, 16
    elev = _dev(_elev("noise", H, W))
    bytes_ = [torch.full((H, W), 77, dtype=torch.uint8, device=DEV) for _ in range(2)]
    d_in, d_out = bytes_
    ints = [torch.full((H, W), 77, dtype=torch.int32, device=DEV) for _ in range(5)]
    acc, basin, length, labels, rank = ints
    counts = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    table = torch.full((3, 2), 77, dtype=torch.int64, device=DEV)
    nbytes = lib.fg_flow_scratch_bytes(H, W)
    assert nbytes == 20 * H * W
    scratch = torch.full((nbytes // 8,), 77, dtype=torch.int64, device=DEV)
    st, null, p = L.stream_handle(), C.c_void_p(0), L.ptr
    odd = lambda t: C.c_void_p(t.data_ptr() + 2)                                   # noqa: E731
    refused = [
        lib.fg_flow_directions(null, H, W, p(d_out), st),
        lib.fg_flow_directions(p(elev), H, W, null, st),
        lib.fg_flow_directions(p(elev), 0, W, p(d_out), st),
        lib.fg_flow_directions(p(elev), 65536, 32768, p(d_out), st),
        lib.fg_flow_directions(odd(elev), H, W, p(d_out), st),
        lib.fg_flow_flats(p(elev), H, W, p(d_in), p(d_out), -1, p(counts), st),
        lib.fg_flow_flats(p(elev), H, W, p(d_in), p(d_out), 32769, p(counts), st),
        lib.fg_flow_flats(p(elev), H, W, p(d_in), p(d_out), 2, null, st),
        lib.fg_flow_flats(p(elev), H, W, p(d_in), p(d_in), 2, p(counts), st),
        lib.fg_flow_flats(p(elev), H, W, null, p(d_out), 2, p(counts), st),
        lib.fg_flow_flats(null, H, W, p(d_in), p(d_out), 2, p(counts), st),
        lib.fg_flow_flats(p(elev), H, -3, p(d_in), p(d_out), 2, p(counts), st),
        lib.fg_flow_flats(p(elev), H, W, p(d_in), p(d_out), 2, odd(counts), st),
        lib.fg_flow_accumulate(p(d_in), H, W, p(acc), p(basin), p(length), null, st),
        lib.fg_flow_accumulate(null, H, W, p(acc), p(basin), p(length), p(scratch), st),
        lib.fg_flow_accumulate(p(d_in), H, W, p(acc), p(acc), p(length), p(scratch), st),
        lib.fg_flow_accumulate(p(d_in), H, W, odd(acc), p(basin), p(length), p(scratch), st),
        lib.fg_flow_accumulate(p(d_in), H, W, p(acc), p(basin), p(length), C.c_void_p(scratch.data_ptr() + 4), st),
        lib.fg_flow_accumulate(p(d_in), 65536, 32768, p(acc), p(basin), p(length), p(scratch), st),
        lib.fg_flow_region_table(p(labels), p(rank), p(acc), p(d_in), H, W, p(table), 0, st),
        lib.fg_flow_region_table(p(labels), p(rank), p(acc), p(d_in), H, W, p(table), H * W + 1, st),
        lib.fg_flow_region_table(p(labels), p(rank), null, p(d_in), H, W, p(table), 3, st),
        lib.fg_flow_region_table(p(labels), p(rank), p(acc), p(d_in), H, W, C.c_void_p(table.data_ptr() + 4), 3, st),
        lib.fg_flow_region_table(p(labels), p(rank), p(acc), p(d_in), 0, W, p(table), 3, st),
    ]
    assert refused == [-1] * len(refused)                     # FG_ERR_INVALID
    assert b"sizes must be positive" in lib.fg_last_error()
    # the Python wrappers: wrong dtype, non-contiguous, R = -1 and R = 32769
    with pytest.raises(RuntimeError, match="the elevation is a contiguous"):
        ops.flow_directions(elev.double(), d_out)
    with pytest.raises(RuntimeError, match="the elevation is a contiguous"):
        ops.flow_directions(elev.t(), d_out)
    with pytest.raises(RuntimeError, match="direction plane is a contiguous"):
        ops.flow_accumulate(acc, acc, basin, length)
    with pytest.raises(RuntimeError, match="32769 rounds"):
        ops.flow_flats(elev, d_in, 32769, d_out, torch.full((32769,), 77, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="-1 rounds"):
        ops.flow_flats(elev, d_in, -1, d_out, counts[:0])
    for bad in (-1, 32769):
        with pytest.raises(ValueError, match="must be 0 .. 32768"):
            flow.flow_directions(elev, flat_rounds=bad)
    with pytest.raises(ValueError, match="must be a torch.float32 tensor"):
        flow.flow_accumulation(elev.double())
    with pytest.raises(ValueError, match="must be contiguous"):
        flow.flow_accumulation(elev.t())
    with pytest.raises(ValueError, match="must be contiguous"):
        flow.flow_accumulation(directions=d_in.t())
    torch.cuda.synchronize()
    for t in bytes_ + ints + [counts, table, scratch]:
        assert bool((t == 77).all())
    # and the same buffers take an accepted call
    want = _oracle("noise", H, W, 3)
    ops.flow_directions(elev, d_in)
    ops.flow_flats(elev, d_in, 3, d_out, counts[:3])
    ops.flow_accumulate(d_out, acc, basin, length)
    assert np.array_equal(d_out.cpu().numpy(), want["directions"])
    assert np.array_equal(counts.cpu().numpy(), np.append(want["flat_directed"], 77))
    assert np.array_equal(acc.cpu().numpy(), want["accumulation"])
    assert np.array_equal(d_in.cpu().numpy(), _oracle("noise", H, W, 0)["directions"])        # flow_flats kept it


def test_an_even_and_an_odd_number_of_rounds_and_none_land_in_the_output():
    from floodgan import ops
    name, H, W = "terraces", 41, 53
    elev, z = _dev(_elev(name, H, W)), _elev(name, H, W)
    d0 = ops.flow_directions(elev, torch.empty((H, W), dtype=torch.uint8, device=DEV))
    for R in (0, 1, 2, 5, 8):
        want, directed = FO.flats(z, FO.directions(z), R)
        out, counts = ops.flow_flats(elev, d0, R, torch.full((H, W), 77, dtype=torch.uint8, device=DEV),
                                     torch.full((R,), 77, dtype=torch.int32, device=DEV))
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), directed), R


# ---- the region table

@pytest.mark.parametrize("H,W", [(41, 53), (96, 130), (33, 64)])
def test_flow_region_table_equals_numpy(H, W):
    from floodgan import ops
    from floodgan.flow import flow_region_table
    from floodgan.regions import rank_plane
    fl = _oracle("terraces", H, W, 3)
    acc, d = _dev(fl["accumulation"]), _dev(fl["directions"])
    for name in ("bernoulli_0.593", "bernoulli_0.3", "frame_island", "flood", "checkerboard"):
        lab = RO.label_class(RO.PATTERNS[name](H, W), True, 8)
        want = FO.region_table(lab, fl["accumulation"], fl["directions"])
        labels = _dev(lab)
        R, rank = rank_plane(labels)
        assert R == len(want["max_accumulation"]) > 0
        table = ops.flow_region_table(labels, rank, acc, d, torch.full((R, 2), 77, dtype=torch.int64, device=DEV))
        assert np.array_equal(table[:, 0].cpu().numpy(), want["max_accumulation"]), name
        assert np.array_equal(table[:, 1].cpu().numpy(), want["pit_pixels"]), name
        regions = {"labels": labels, "table": RO.table(lab)}
        got = flow_region_table({"accumulation": acc, "directions": d}, regions)
        assert set(got) == {"max_accumulation", "pit_pixels"}
        for col in got:
            assert got[col].dtype == np.int64 and np.array_equal(got[col], want[col]), (name, col)
    assert want["pit_pixels"].sum() > 0 and want["max_accumulation"].max() > 8


# ---- predict_scene

class _Identity(torch.nn.Module):
    def forward(self, x):
        return x[:, :3]


def _patch_unet(monkeypatch):
    """predict_scene's U-Net path replaced by a known logit pattern (tests/test_gpu_depth.py): +4 where the picture's
    first channel is positive, -4 elsewhere, so `> 0` on the host is the device's decision after the blend."""
    from floodgan import scene
    monkeypatch.setattr(scene, "_unet", lambda seg_model, batch_stats: seg_model)
    monkeypatch.setattr(scene, "_flood_logits",
                        lambda unet, images, batch_stats: torch.where(images[:, :1] > 0, 4.0, -4.0))


def test_predict_scene_gains_the_flow_only_when_asked(monkeypatch):
    from floodgan.scene import predict_scene
    _patch_unet(monkeypatch)
    H, W, tile, overlap = 48, 56, 16, 8
    mask = RO.bernoulli(H, W, 0.5, 5)
    x = torch.from_numpy(np.where(mask, 0.5, -0.5).astype(np.float32))[None, None].repeat(1, 3, 1, 1).to(DEV)
    z = FO.PATTERNS["terraces"](H, W)
    elev = _dev(z)
    want = FO.flow(z, 3)
    common = dict(tile=tile, overlap=overlap, batch=5)
    # without a segmentation model: the picture and the flow
    alone = predict_scene(_Identity(), x, elevation=elev, drainage=True, flat_rounds=3, **common)
    assert set(alone) == {"grid", "output", "flow"}
    _same_flow(alone["flow"], want, "no seg_model")
    # with one: the elevation's depth keys as before, the flow, and the two columns in the regions' table
    plain = predict_scene(_Identity(), x, seg_model="stub", elevation=elev, connectivity=4, **common)
    assert set(plain) == {"grid", "output", "flood_logits", "flood_fraction", "flood_mask", "regions", "flood_depth",
                          "depth"}                                                   # the keys before, exactly
    assert set(plain["regions"]["table"]) == set(RO.COLUMNS)
    res = predict_scene(_Identity(), x, seg_model="stub", elevation=elev[None, None], connectivity=4, drainage=True,
                        flat_rounds=3, **common)
    assert set(res) == set(plain) | {"flow"}
    for key in ("output", "flood_logits", "flood_mask", "flood_depth"):
        assert torch.equal(res[key], plain[key]), key
    assert torch.equal(res["regions"]["labels"], plain["regions"]["labels"])
    regions = RO.flood_regions(mask, 1, 0, 4)
    assert np.array_equal(res["regions"]["labels"].cpu().numpy(), regions["labels"]) and regions["count"] > 3
    table = FO.region_table(regions["labels"], want["accumulation"], want["directions"])
    flow = dict(res["flow"])
    assert set(flow.pop("table")) == {"max_accumulation", "pit_pixels"}
    _same_flow(flow, want, "with seg_model")
    assert set(res["regions"]["table"]) == set(RO.COLUMNS) | {"max_accumulation", "pit_pixels"}
    for col in RO.COLUMNS:
        assert np.array_equal(res["regions"]["table"][col], plain["regions"]["table"][col]), col
    for col in ("max_accumulation", "pit_pixels"):
        assert np.array_equal(res["regions"]["table"][col], table[col]), col
        assert np.array_equal(res["flow"]["table"][col], table[col]), col
    with pytest.raises(ValueError, match="needs elevation"):
        predict_scene(_Identity(), x, seg_model="stub", drainage=True, **common)
    with pytest.raises(ValueError, match="needs seg_model"):
        predict_scene(_Identity(), x, elevation=elev, **common)                  # as before: no drainage, no depth


def test_model_predict_scene_writes_the_flow_picture_and_the_columns(tmp_path, monkeypatch):
    from floodgan.model import Model
    from floodgan.outline import write_regions_geojson
    from floodgan.png import read_png
    from floodgan.regions import write_regions_csv
    _patch_unet(monkeypatch)
    root = str(tmp_path)
    H, W = 40, 56
    raw = np.random.default_rng(21).random((H, W, 9)).astype(np.float32)
    raw[:, :, 3] = FO.PATTERNS["terraces"](H, W) / np.float32(100)                   # the elevation, read back * 100
    path = os.path.join(root, "harvey_scene.tif")
    write_tiff(path, raw)
    m = Model(model="PairedAttention", training_model=False, data_path=root, resize=None, crop=None,
              train_loader=[], device=DEV)
    common = dict(tile=32, overlap=8, batch=3)
    files = ("harvey_scene_floodRegions.csv", "harvey_scene_floodRegions.geojson")
    before = m.predict_scene(path, seg_model_path="stub", polygons=True, connectivity=4, **common)
    assert set(before) == {"prediction", "flood_mask", "flood_fraction", "grid", "regions", "region_count",
                           "polygons"}                                               # the keys before, exactly
    assert "flow" not in m.last_scene and not os.path.exists(f"{root}/images/harvey_scene_flowAccumulation.png")
    kept = [open(f"{root}/images/{f}", "rb").read() for f in files]
    # the files without drainage are what the writers give without a flow: the bytes of before this feature
    regions, outlines = m.last_scene["regions"], m.last_scene["outlines"]
    assert set(regions["table"]) == set(RO.COLUMNS)
    write_regions_csv(f"{root}/plain.csv", regions)
    write_regions_geojson(f"{root}/plain.geojson", regions, outlines)
    assert kept == [open(f"{root}/plain.csv", "rb").read(), open(f"{root}/plain.geojson", "rb").read()]
    elev = (raw[:, :, 3] * np.float32(100)).astype(np.float32)
    want = FO.flow(elev, 2)
    assert want["pit_count"] > 0 and want["accumulation"].max() > 8
    written = m.predict_scene(path, seg_model_path="stub", polygons=True, connectivity=4, drainage=True,
                              flat_rounds=2, **common)
    assert set(written) == set(before) | {"flow_accumulation", "pit_count"}
    assert written["flow_accumulation"] == f"{root}/images/harvey_scene_flowAccumulation.png"
    assert written["pit_count"] == want["pit_count"]
    assert "depth" not in m.last_scene                                               # drainage asks for no depth
    flow = dict(m.last_scene["flow"])
    table = flow.pop("table")
    _same_flow(flow, want, "model")
    from floodgan.flow import render_flow
    unit = render_flow(flow["accumulation"]).cpu().numpy()
    assert np.allclose(unit, FO.render(want["accumulation"]), rtol=0, atol=1e-6) and unit.max() <= 1.0
    img, text = read_png(written["flow_accumulation"])
    assert text == {} and img.tobytes() == PO.scalar_bytes(unit, cmap="gray_r", kind="unit").tobytes()
    lab = m.last_scene["regions"]["labels"].cpu().numpy()
    want_table = FO.region_table(lab, want["accumulation"], want["directions"])
    lines_before, lines = kept[0].decode().splitlines(), open(written["regions"]).read().splitlines()
    assert lines[0] == lines_before[0] + ",max_accumulation,pit_pixels" and len(lines) == len(lines_before) > 3
    for r, (a, b) in enumerate(zip(lines_before[1:], lines[1:])):
        assert b == a + f",{want_table['max_accumulation'][r]},{want_table['pit_pixels'][r]}"
    fa, fb = json.loads(kept[1])["features"], json.load(open(written["polygons"]))["features"]
    for r, (a, b) in enumerate(zip(fa, fb)):
        assert b["geometry"] == a["geometry"]
        assert list(b["properties"]) == list(a["properties"]) + ["max_accumulation", "pit_pixels"]
        assert b["properties"]["max_accumulation"] == int(table["max_accumulation"][r]) == \
            int(want_table["max_accumulation"][r])
    # without a segmentation model: the prediction and the flow picture alone
    only = m.predict_scene(path, drainage=True, **common)
    assert set(only) == {"prediction", "flood_mask", "flood_fraction", "grid", "flow_accumulation", "pit_count"}
    assert only["flood_mask"] is None and only["pit_count"] == FO.flow(elev, 0)["pit_count"]
    write_tiff(os.path.join(root, "rgb.tif"), raw[:, :, :3].copy())
    with pytest.raises(ValueError, match="has 3 channels"):
        m.predict_scene(os.path.join(root, "rgb.tif"), drainage=True, **common)
    with pytest.raises(ValueError, match="must be 0 .. 32768"):
        m.predict_scene(path, drainage=True, flat_rounds=-1, **common)
