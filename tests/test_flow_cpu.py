"""The flow routing's semantics without a device: the numpy oracle (tests/flow_oracle.py) against a step-by-step walk
and the four identities of DESIGN.md §21, the direction rule against exact rational slopes, the conditions the GPU
tests' inputs have to meet, render_flow, the CSV / GeoJSON columns, the option errors and the new names."""
import functools
import itertools
from fractions import Fraction

import numpy as np
import pytest

import flow_oracle as FO
import regions_oracle as RO

SHAPES = [(1, 1), (1, 37), (37, 1), (16, 16), (41, 53)]


@functools.lru_cache(maxsize=None)
def _flow(name, H, W, R):
    z = FO.PATTERNS[name](H, W)
    res = FO.flow(z, R)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return z, res


def _check_identities(z, res, walk):
    d, acc, basin, length = (res[k] for k in ("directions", "accumulation", "basin", "length"))
    H, W = d.shape
    data = np.isfinite(z)
    assert d.dtype == np.uint8 and acc.dtype == basin.dtype == length.dtype == np.int32
    assert np.array_equal(d == FO.NODATA, ~data) and res["nodata_count"] == int((~data).sum())
    recv = FO.receivers(d)
    a, b, ln = acc.ravel(), basin.ravel(), length.ravel()
    has = recv >= 0
    # acc[p] = 1 + the sum over p's children
    children = np.zeros(H * W, dtype=np.int64)
    np.add.at(children, recv[has], a[has])
    assert np.array_equal(a[data.ravel()], 1 + children[data.ravel()]) and not a[~data.ravel()].any()
    pits = np.flatnonzero(d.ravel() == FO.PIT)
    assert np.array_equal(np.flatnonzero(data.ravel() & ~has), pits) and res["pit_count"] == len(pits)
    assert int(a[pits].sum()) == int(data.sum())
    assert np.array_equal(a[pits], np.bincount(b[b >= 0], minlength=H * W)[pits])
    assert np.array_equal(ln[has], ln[recv[has]] + 1) and not ln[pits].any()
    assert np.array_equal(b[has], b[recv[has]]) and np.array_equal(b[pits], pits)
    assert (b[~data.ravel()] == -1).all() and (ln[~data.ravel()] == -1).all()
    for p in walk:
        if data.ravel()[p]:
            assert FO.follow(recv, p) == (b[p], ln[p]), p


@pytest.mark.parametrize("R", [0, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_the_oracle_meets_the_walk_and_the_identities(H, W, R):
    for name in FO.PATTERNS:
        z, res = _flow(name, H, W, R)
        assert res["rounds"] == int(np.ceil(np.log2(max(H * W, 2))))
        _check_identities(z, res, range(H * W) if H * W <= 16 * 16 else range(0, H * W, 7))


def test_the_identities_at_96_x_130():
    for name in FO.PATTERNS:
        z, res = _flow(name, 96, 130, 64 if name == "terraces" else 0)
        _check_identities(z, res, range(0, 96 * 130, 101))


def test_round_zero_directions_strictly_descend_and_flats_stay_level():
    for name, R in itertools.product(("terraces", "noise", "holes", "cone"), (0, 64)):
        z, res = _flow(name, 41, 53, R)
        d0 = FO.directions(z)
        recv = FO.receivers(res["directions"])
        zz, has = z.ravel(), recv >= 0
        steep = has & (d0.ravel() < 8)
        assert np.array_equal(res["directions"].ravel()[steep], d0.ravel()[steep])        # the wave keeps round 0
        assert (zz[steep] > zz[recv[steep]]).all()
        assert (zz[has & ~steep] == zz[recv[has & ~steep]]).all()


def _fraction_direction(z, y, x):
    """the D8 code of pixel (y, x) by exact rational arithmetic on the squared slopes d^2 / dist^2"""
    H, W = z.shape
    best, code = Fraction(0), FO.PIT
    for k, (dy, dx) in enumerate(FO.NEIGHBOURS):
        yn, xn = y + dy, x + dx
        if not (0 <= yn < H and 0 <= xn < W):
            continue
        d = Fraction(float(z[y, x])) - Fraction(float(z[yn, xn]))          # exact: the test values subtract exactly
        if d > 0 and d * d / (dy * dy + dx * dx) > best:
            best, code = d * d / (dy * dy + dx * dx), k
    return code


def test_the_direction_rule_equals_exact_rational_slopes_on_a_tie_set():
    """5 x 7 planes over a small set of levels: every pixel sees ties between cardinals, between diagonals and none
    between the two kinds but through the key (2 d^2 against d^2: 1 cardinal step of 1 loses to no diagonal step
    below sqrt(2), so 1 against 1.5 and 2 against 3 are decided by the squares)."""
    levels = np.array([0.0, 1.0, 1.5, 2.0, 3.0, 4.0], dtype=np.float32)
    rng = np.random.default_rng(5)
    planes = [levels[rng.integers(0, len(levels), (5, 7))] for _ in range(40)]
    # and the exhaustive neighbourhoods of one centre pixel over three levels: 3^8 rings around a centre of 2
    ring = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)]
    for combo in itertools.product((0.0, 1.0, 1.5), repeat=8):
        p = np.full((3, 3), 2.0, dtype=np.float32)
        for (y, x), v in zip(ring, combo):
            p[y, x] = v
        assert FO.directions(p)[1, 1] == _fraction_direction(p, 1, 1), combo
    for z in planes:
        d = FO.directions(z)
        for y in range(5):
            for x in range(7):
                assert d[y, x] == _fraction_direction(z, y, x), (z, y, x)
    # hand-checked: a diagonal drop of 1.5 beats a cardinal drop of 1 (2.25 > 2), one of 1 does not (1 < 2)
    z = np.array([[9, 9, 9], [9, 2, 1], [9, 9, 0.5]], dtype=np.float32)
    assert FO.directions(z)[1, 1] == 1
    z[2, 2] = 1.0
    assert FO.directions(z)[1, 1] == 0
    z[1, 2] = 2.0
    z[1, 0] = 1.0
    assert FO.directions(z)[1, 1] == 4                          # cardinal W (k 4) against diagonal SE (k 1): 2 > 1


def test_the_conditions_the_gpu_inputs_have_to_meet():
    z = FO.PATTERNS["terraces"](96, 130)
    d0 = FO.directions(z)
    pits = {}
    for R in (0, 3, 64):
        d, directed = FO.flats(z, d0, R)
        pits[R] = int((d == FO.PIT).sum())
    assert pits[64] < pits[3] < pits[0]
    assert directed[0] > 0 and (directed == 0).any() and int(np.flatnonzero(directed == 0)[0]) < 63
    assert FO.flats(z, d0, 3)[1].tolist() == directed[:3].tolist()
    _, res = _flow("spiral", 257, 515, 0)
    assert res["length"].max() >= 2 ** 16 and res["pit_count"] == 1
    assert res["rounds"] == 18 and 2 ** 17 < 257 * 515 <= 2 ** 18
    z, res = _flow("noise", 96, 130, 0)
    assert res["pit_count"] > 500
    ulp = np.abs(np.diff(z.view(np.int32), axis=1)) == 1
    assert ulp.sum() > 100                                      # neighbours one ulp apart
    z, res = _flow("constant", 16, 16, 3)
    assert res["pit_count"] == 256 and not res["flat_directed"].any()
    z, res = _flow("checkerboard", 16, 16, 0)
    assert res["pit_count"] == 128 and set(res["directions"][RO.checkerboard(16, 16)].tolist()) <= {0, 2, 4, 6}
    z, res = _flow("holes", 41, 53, 0)
    assert res["nodata_count"] > 41 and np.isinf(z).sum() == 2
    for name in ("ramp_x", "ramp_diag"):
        _, res = _flow(name, 41, 53, 0)
        assert res["length"].max() >= 52
    _, res = _flow("cone", 41, 53, 0)
    assert res["pit_count"] == 1 and res["accumulation"].max() == 41 * 53


def test_render_flow():
    import torch

    from floodgan.flow import render_flow
    _, res = _flow("cone", 41, 53, 0)
    acc = torch.from_numpy(res["accumulation"].copy())
    out = render_flow(acc)
    assert out.dtype == torch.float32 and tuple(out.shape) == (41, 53)
    assert float(out.min()) == 0.0 and float(out.max()) == 1.0                 # leaves and the one pit
    assert np.allclose(out.numpy(), FO.render(res["accumulation"]), rtol=0, atol=2e-7)
    half = render_flow(acc, vmax=64)
    assert float(half.max()) == 1.0 and np.allclose(half.numpy(), FO.render(res["accumulation"], 64), atol=2e-7)
    assert float(half[acc == 8][0]) == 0.5                                     # log2 8 / log2 64
    assert not render_flow(torch.zeros((3, 4), dtype=torch.int32)).any()       # nodata only: vmax 0 -> 2
    with pytest.raises(ValueError, match="integer tensor"):
        render_flow(torch.zeros(3, 4))
    with pytest.raises(ValueError, match="must be positive"):
        render_flow(acc, vmax=0)


def test_the_csv_and_the_geojson_gain_the_flow_columns_only_when_asked(tmp_path):
    import json

    import outline_oracle as OO
    from floodgan.outline import write_regions_geojson
    from floodgan.regions import write_regions_csv
    H, W = 41, 53
    res = RO.flood_regions(RO.bernoulli(H, W, 0.5, 5), 3, 0, 4)
    _, fl = _flow("terraces", H, W, 3)
    flow = dict(fl, table=FO.region_table(res["labels"], fl["accumulation"], fl["directions"]))
    assert flow["table"]["pit_pixels"].sum() > 0 and flow["table"]["max_accumulation"].max() > 8
    plain, with_flow = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    write_regions_csv(plain, res)
    write_regions_csv(str(tmp_path / "a2.csv"), res, None, None)
    assert open(plain, "rb").read() == open(tmp_path / "a2.csv", "rb").read()
    write_regions_csv(with_flow, res, flow=flow)
    a, b = open(plain).read().splitlines(), open(with_flow).read().splitlines()
    assert b[0] == a[0] + ",max_accumulation,pit_pixels" and len(a) == len(b) == res["count"] + 1
    for r, (la, lb) in enumerate(zip(a[1:], b[1:])):
        assert lb == la + f",{flow['table']['max_accumulation'][r]},{flow['table']['pit_pixels'][r]}"
    with pytest.raises(ValueError, match="no table of these regions"):
        write_regions_csv(with_flow, res, flow=fl)
    outlines = OO.outlines(res["labels"], 4)
    ga, gb = str(tmp_path / "a.geojson"), str(tmp_path / "b.geojson")
    write_regions_geojson(ga, res, outlines)
    write_regions_geojson(str(tmp_path / "a2.geojson"), res, outlines, None, None, None)
    assert open(ga, "rb").read() == open(tmp_path / "a2.geojson", "rb").read()
    write_regions_geojson(gb, res, outlines, flow=flow)
    fa, fb = json.load(open(ga))["features"], json.load(open(gb))["features"]
    assert len(fa) == len(fb) == res["count"] > 3
    for r, (x, y) in enumerate(zip(fa, fb)):
        assert y["geometry"] == x["geometry"]
        assert list(y["properties"]) == list(x["properties"]) + ["max_accumulation", "pit_pixels"]
        assert {k: y["properties"][k] for k in x["properties"]} == x["properties"]
        assert y["properties"]["max_accumulation"] == int(flow["table"]["max_accumulation"][r])
        assert y["properties"]["pit_pixels"] == int(flow["table"]["pit_pixels"][r])
    with pytest.raises(ValueError, match="no table of these regions"):
        write_regions_geojson(gb, res, outlines, flow=fl)


def test_option_refusals_come_before_any_launch():
    import torch

    from floodgan.flow import flow_accumulation, flow_directions
    from floodgan.scene import predict_scene
    cpu = torch.zeros(4, 5)

    class Cuda(torch.Tensor):                    # passes the device checks without a device
        is_cuda = True

    with pytest.raises(ValueError, match="must be on a HIP device"):
        flow_directions(cpu)
    with pytest.raises(ValueError, match="must be a torch.float32 tensor"):
        flow_directions(torch.zeros(4, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="must be a torch.float32 tensor"):
        flow_directions(np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="must be \\[H, W\\] or \\[1, 1, H, W\\]"):
        flow_directions(torch.zeros(1, 3, 4, 5))
    with pytest.raises(ValueError, match="must be contiguous"):
        flow_directions(torch.zeros(5, 4).t().as_subclass(Cuda))
    with pytest.raises(ValueError, match="below 2\\^31"):
        flow_directions(torch.zeros(1).expand(65536, 32768).as_subclass(Cuda))
    for bad in (-1, 32769):
        with pytest.raises(ValueError, match="must be 0 .. 32768"):
            flow_directions(cpu, flat_rounds=bad)
        with pytest.raises(ValueError, match="must be 0 .. 32768"):
            flow_accumulation(cpu, flat_rounds=bad)
    with pytest.raises(ValueError, match="must be an integer"):
        flow_directions(cpu, flat_rounds=1.5)
    with pytest.raises(ValueError, match="exactly one of"):
        flow_accumulation()
    with pytest.raises(ValueError, match="exactly one of"):
        flow_accumulation(cpu, directions=torch.zeros(4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="must be a torch.uint8 tensor"):
        flow_accumulation(directions=cpu)
    with pytest.raises(ValueError, match="taken as it is"):
        flow_accumulation(directions=torch.zeros(4, 5, dtype=torch.uint8), flat_rounds=2)
    x = torch.zeros(1, 3, 16, 16).as_subclass(Cuda)
    with pytest.raises(ValueError, match="drainage=True .* needs elevation"):
        predict_scene(lambda t: t, x, tile=16, overlap=0, drainage=True)
    with pytest.raises(ValueError, match="drainage=True .* needs elevation"):
        predict_scene(lambda t: t, torch.zeros(1, 3, 16, 16), tile=16, overlap=0, seg_model="stub", drainage=True)
    with pytest.raises(ValueError, match="must be 0 .. 32768"):
        predict_scene(lambda t: t, x, tile=16, overlap=0, drainage=True, elevation=torch.zeros(16, 16),
                      flat_rounds=40000)
    with pytest.raises(ValueError, match="elevation must be a float32 \\[16, 16\\]"):
        predict_scene(lambda t: t, x, tile=16, overlap=0, drainage=True, elevation=torch.zeros(16, 17))


def test_new_names_are_exported():
    import inspect

    import floodgan
    from floodgan import _lib as L, flow, model, ops, outline, regions, scene
    for name in ("flow_directions", "flow_accumulation", "render_flow"):
        assert name in floodgan.__all__ and getattr(floodgan, name) is getattr(flow, name)
    assert {"fg_flow_directions", "fg_flow_flats", "fg_flow_accumulate", "fg_flow_scratch_bytes", "fg_flow_rounds",
            "fg_flow_region_table"} <= set(L.SIGNATURES)
    for name in ("flow_directions", "flow_flats", "flow_accumulate", "flow_region_table"):
        assert callable(getattr(ops, name))
    p = inspect.signature(flow.flow_accumulation).parameters
    assert p["elevation"].default is None and p["directions"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["flat_rounds"].default == 0 and inspect.signature(flow.flow_directions).parameters["flat_rounds"].default == 0
    for fn in (scene.predict_scene, model.Model.predict_scene):
        p = inspect.signature(fn).parameters
        assert p["drainage"].default is False and p["flat_rounds"].default == 0
    assert inspect.signature(regions.write_regions_csv).parameters["flow"].default is None
    assert inspect.signature(outline.write_regions_geojson).parameters["flow"].default is None
    assert regions.FLOW_COLUMNS == flow.FLOW_TABLE_COLUMNS == ("max_accumulation", "pit_pixels")
    assert flow.NEIGHBOURS == FO.NEIGHBOURS and (flow.PIT, flow.NODATA) == (FO.PIT, FO.NODATA)


def test_the_library_sizes_its_rounds_and_scratch_on_the_host():
    from floodgan import _lib as L
    lib = L.load()
    sizes = [(1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (16, 16), (41, 53), (257, 515), (32768, 65535)]
    assert [lib.fg_flow_rounds(H, W) for H, W in sizes] == [1, 1, 2, 2, 3, 8, 12, 18, 31]
    assert [lib.fg_flow_rounds(H, W) for H, W in sizes] == [FO.rounds(H, W) for H, W in sizes]
    assert lib.fg_flow_scratch_bytes(16, 16) == 20 * 256 and lib.fg_flow_scratch_bytes(1, 37) == 5 * 152
    assert lib.fg_flow_scratch_bytes(0, 4) == lib.fg_flow_scratch_bytes(65536, 32768) == 0
    assert lib.fg_flow_rounds(4, -1) == lib.fg_flow_rounds(65536, 32768) == 0
