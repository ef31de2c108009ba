"""The flood depth on the HIP path (csrc/distance.hip through floodgan.depth) against the numpy oracle
(tests/depth_oracle.py).  The transform and the table are integers, the depth is one fp32 subtraction of exactly
representable values: every comparison is exact equality.

Tile arithmetic.  The column pass works in bands of 64 rows: 96 crosses one band border, 257 four (64, 128, 192, 256)
and leaves a band of one row.  The row pass works in segments of 256 columns and stages the row in chunks of 256: 515
crosses two borders and leaves a segment of three columns, and a pixel of its first segment searches three rings (the
two LDS slots of a side are both reused); 1100 columns (five segments, five rings) reuse each slot twice.  No shape is
a multiple of either."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import depth_oracle as DO
import regions_oracle as RO
import render_oracle as PO
from tiff_util import write_tiff

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 1), (1, 37), (37, 1), (16, 16), (41, 53), (96, 130)]
BIG = (257, 515)
BIG_PATTERNS = ["flood", "checkerboard", "spiral", "bernoulli_0.593"]
CASES = [(H, W, name) for H, W in SHAPES for name in RO.PATTERNS] + [BIG + (name,) for name in BIG_PATTERNS]
OWN_SHAPES = [(96, 130), BIG, (5, 1100)]
# (the list of tests/test_gpu_regions.py) +0, -0, NaN, the negatives and -inf are dry; 2^-20, 88 and +inf are flood
SPECIALS = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 88.0, -88.0, float("inf"), float("-inf"), float("nan")]
FLOOD_SPECIALS, DRY_SPECIALS = [2, 4, 6], [0, 1, 3, 5, 7, 8]
DEPTH_MASKS = ["frame_island", "spiral", "bernoulli_0.593", "flood", "dry"]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from floodgan import _lib as L
    L.load()


def _own_planes(H, W):
    """the seed planes of this feature's own: name -> boolean [H, W]"""
    def at(*pixels):
        m = np.zeros((H, W), dtype=bool)
        for y, x in pixels:
            m[y, x] = True
        return m
    cy, cx = H // 2, W // 2
    last_col, last_row = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    last_col[H // 3, W - 1] = True
    last_row[H - 1, W // 3] = True
    first_row, first_col = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    first_row[0] = True
    first_col[:, 0] = True
    return {"top_left": at((0, 0)), "top_right": at((0, W - 1)), "bottom_left": at((H - 1, 0)),
            "bottom_right": at((H - 1, W - 1)), "centre": at((cy, cx)), "last_column": last_col, "last_row": last_row,
            "about_a_column": at((cy, cx - 2), (cy, cx + 2)), "about_a_row": at((cy - 2, cx), (cy + 2, cx)),
            "about_a_diagonal": at((cy - 2, cx + 2), (cy + 2, cx - 2)) if H > 4 else at((0, cx + 2), (H - 1, cx - 2)),
            "first_row": first_row, "first_column": first_col,
            "all": np.ones((H, W), dtype=bool), "none": np.zeros((H, W), dtype=bool)}


@functools.lru_cache(maxsize=None)
def _seeds(H, W, name):
    m = RO.PATTERNS[name](H, W) if name in RO.PATTERNS else _own_planes(H, W)[name]
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _oracle(H, W, name, target):
    m = _seeds(H, W, name)
    near, d2 = DO.nearest_seed_separable(m if target else ~m)
    near.setflags(write=False)
    d2.setflags(write=False)
    return near, d2


def _values(mask, kind, seed=0):
    """a float32 [H, W] numpy plane whose class under `kind` is mask"""
    if kind == "threshold":
        return mask.astype(np.float32)
    sp = np.array(SPECIALS, dtype=np.float32)
    pick = np.random.default_rng(seed).integers(0, 1 << 30, mask.shape)
    return np.where(mask, sp[np.array(FLOOD_SPECIALS)][pick % 3], sp[np.array(DRY_SPECIALS)][pick % 6])


def _dev(values):
    return torch.from_numpy(np.ascontiguousarray(values))[None, None].to(DEV)


def _check_planes(got, want, what):
    near, d2 = got
    assert near.dtype == torch.int32 and d2.dtype == torch.int32 and near.is_cuda and d2.is_cuda, what
    assert tuple(near.shape) == tuple(d2.shape) == want[0].shape, what
    assert np.array_equal(near.cpu().numpy(), want[0]), what
    assert np.array_equal(d2.cpu().numpy(), want[1]), what


@pytest.mark.parametrize("kind", ["threshold", "logit"])
@pytest.mark.parametrize("H,W", SHAPES + [BIG])
def test_nearest_seed_equals_the_oracle(H, W, kind):
    from floodgan.depth import nearest_seed
    for name in [n for h, w, n in CASES if (h, w) == (H, W)]:
        src = _dev(_values(_seeds(H, W, name), kind, seed=H + W))
        for target in (True, False):
            _check_planes(nearest_seed(src, kind, target), _oracle(H, W, name, target), (name, target))


@pytest.mark.parametrize("H,W", OWN_SHAPES)
def test_single_seeds_ties_and_the_extremes(H, W):
    from floodgan.depth import nearest_seed
    for name in _own_planes(H, W):
        src = _dev(_values(_seeds(H, W, name), "threshold"))
        want = _oracle(H, W, name, True)
        _check_planes(nearest_seed(src, "threshold", True), want, name)
        if name == "top_left":
            assert want[1][H - 1, W - 1] == (H - 1) ** 2 + (W - 1) ** 2           # the search ran the whole scene
        if name == "about_a_column":
            assert want[0][H // 2, W // 2] == (H // 2) * W + W // 2 - 2            # the tie goes to the smaller index
        if name == "none":
            assert (want[0] == -1).all() and (want[1] == -1).all()
    # the dry class of the single corner seed: every pixel but one is a seed
    src = _dev(_values(_seeds(H, W, "top_left"), "logit", seed=3))
    _check_planes(nearest_seed(src, "logit", False), _oracle(H, W, "top_left", False), "complement")


def _forms(values):
    """a float32 [H, W] numpy plane in the forms the kernels read"""
    from floodgan.plans import Buf
    H, W = values.shape
    t = torch.from_numpy(values.copy()).to(DEV)
    wide = torch.full((1, 3, H, W), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)
    wide[0, 0] = t
    assert wide.stride(3) == 3 and wide.stride(1) == 1
    buf = Buf.empty(1, H, W, 4, 0, DEV)
    buf.t.fill_(7.0)
    buf.interior()[0, :, :, 0] = t
    return {"plane": t, "nchw": t[None, None], "channels_last": wide, "buf": buf}


@pytest.mark.parametrize("kind", ["threshold", "logit"])
def test_every_input_form_gives_the_same_planes(kind):
    from floodgan.depth import nearest_seed
    H, W, name = 96, 130, "bernoulli_0.3"
    values = _values(_seeds(H, W, name), kind, seed=5)
    if kind == "threshold":
        rng = np.random.default_rng(11)
        values = np.where(values > 0, rng.uniform(0.51, 2.0, (H, W)), rng.uniform(-2.0, 0.5, (H, W))).astype(np.float32)
    for form, src in _forms(values).items():
        for target in (True, False):
            _check_planes(nearest_seed(src, kind, target), _oracle(H, W, name, target), (form, target))


def test_two_calls_are_bit_identical_and_dist2_is_optional():
    from floodgan.depth import nearest_seed
    H, W, name = BIG + ("bernoulli_0.593",)
    src = _dev(_values(_seeds(H, W, name), "threshold"))
    a, b = nearest_seed(src, "threshold", False), nearest_seed(src, "threshold", False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    near, none = nearest_seed(src, "threshold", False, dist2=False)
    assert none is None and torch.equal(near, a[0])


# ---- depth

def _elevation(H, W, special):
    """multiples of 2^-10 in [0, 64): every difference and every quantum is exact.  special: NaN and the infinities
    planted on a regular grid (it meets shore and interior pixels of every mask used here)."""
    e = (np.random.default_rng(1000 * H + W).integers(0, 65536, (H, W)) / 1024.0).astype(np.float32)
    if special:
        flat = e.ravel()
        flat[5::29] = np.nan
        flat[11::31] = np.inf
        flat[17::37] = -np.inf
    return e


@functools.lru_cache(maxsize=None)
def _oracle_depth(H, W, name, sieve, special):
    regions = RO.flood_regions(_seeds(H, W, name), 8 if sieve else 1, 8 if sieve else 0, 8)
    return regions, DO.flood_depth(regions["mask"], _elevation(H, W, special), regions["labels"],
                                   regions["table"]["area"], pixel_area=0.25)


def _same_depth(got, want, what, table=True):
    assert got["depth"].dtype == torch.float32 and tuple(got["depth"].shape) == (1, 1) + want["depth"].shape, what
    assert got["depth"][0, 0].cpu().numpy().tobytes() == want["depth"].tobytes(), what
    assert got["nearest_shore"].dtype == torch.int32, what
    assert np.array_equal(got["nearest_shore"].cpu().numpy(), want["nearest_shore"]), what
    for key in ("shore_count", "wet_area", "max_depth", "mean_depth", "volume"):
        assert got[key] == want[key] and type(got[key]) is type(want[key]), (what, key)
    if table:
        assert set(got["table"]) == set(want["table"]), what
        for col in ("wet_area", "depth_sum_q", "depth_max_q"):
            assert got["table"][col].dtype == np.int64 and np.array_equal(got["table"][col], want["table"][col]), \
                (what, col)
        for col in ("mean_depth", "max_depth", "volume"):
            assert got["table"][col].dtype == np.float64 and np.array_equal(got["table"][col], want["table"][col]), \
                (what, col)
    else:
        assert "table" not in got, what


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("sieve", [False, True])
@pytest.mark.parametrize("H,W", [(41, 53), (96, 130)])
def test_flood_depth_equals_the_oracle(H, W, sieve, special):
    from floodgan.depth import flood_depth
    from floodgan.regions import flood_regions
    elev = torch.from_numpy(_elevation(H, W, special)).to(DEV)
    planted = 0
    for name in DEPTH_MASKS:
        want_regions, want = _oracle_depth(H, W, name, sieve, special)
        regions = flood_regions(_dev(_values(_seeds(H, W, name), "threshold")), "threshold", 8 if sieve else 1,
                                8 if sieve else 0, 8)
        assert np.array_equal(regions["labels"].cpu().numpy(), want_regions["labels"]), name
        got = flood_depth(regions["mask"], elev, regions, pixel_area=0.25)
        _same_depth(got, want, (name, H, W, sieve, special))
        if name in ("flood", "dry"):
            assert got["shore_count"] == 0 and got["max_depth"] == 0.0 and not bool(got["depth"].any())
            assert bool((got["nearest_shore"] == -1).all())
        elif special:
            e, s = _elevation(H, W, True), DO.shore(want_regions["mask"])
            planted += int((~np.isfinite(e) & s).sum() > 0) + int((~np.isfinite(e) & want_regions["mask"] & ~s).sum() > 0)
        # without the regions: the same planes and totals, no table; the elevation as [1, 1, H, W]
        if name == "frame_island":
            _same_depth(flood_depth(regions["mask"][0, 0], elev[None, None], pixel_area=0.25), want, name, table=False)
    if special:
        assert planted >= 4                 # NaN / infinities sat on shore and on interior pixels
    if (H, W, sieve, special) == (96, 130, False, False):
        _, want = _oracle_depth(H, W, "frame_island", False, False)
        assert want["wet_area"] > 300 and want["table"]["wet_area"].min() > 0 and want["max_depth"] > 32


# ---- the accumulation kernel behind the three tables (csrc/scene_common.hpp)

@functools.lru_cache(maxsize=None)
def _oracle_tables(H, W, name):
    """(labels, region table, depth plane, depth table, the scene's depth row) of a pattern.  The depths hold zeros,
    values that round to no quantum (2^-11 is a tie to even), negatives, ordinary values and values above the 2^20
    cap."""
    lab = RO.label_class(_seeds(H, W, name), True, 8)
    values = np.array([0.0, 2.0 ** -12, 2.0 ** -11, 3 * 2.0 ** -11, -1.0, 0.5, 37.25, 2.0 ** 20, 2.0 ** 21],
                      dtype=np.float32)
    d = values[np.random.default_rng(H * W).integers(0, len(values), (H, W))]
    q = DO.quanta(d)
    scene = np.array([(q > 0).sum(), q[q > 0].sum(), q.max()], dtype=np.int64)
    for a in (lab, d):
        a.setflags(write=False)
    return lab, RO.table(lab), d, DO.depth_table(lab, d), scene


def _placed(values, shift):
    """values [H, W] as a contiguous device view that starts `shift` elements into a fresh buffer"""
    H, W = values.shape
    host = torch.from_numpy(values.copy())
    buf = torch.empty(H * W + 4, dtype=host.dtype, device=DEV)
    view = buf[shift:shift + H * W].view(H, W)
    view.copy_(host)
    assert view.is_contiguous() and view.data_ptr() % 16 == values.itemsize * shift
    return view


@pytest.mark.parametrize("H,W", [(33, 64), (16, 16)])
def test_the_three_tables_take_a_16_byte_and_a_4_byte_aligned_labels_plane(H, W):
    """W is a multiple of the run of 4, so a 16-byte aligned labels plane is read by 16-byte loads and one that starts
    4 bytes later pixel by pixel.  33 x 64 is 528 runs: two full blocks and a third of one partial wave and three
    empty ones, which the whole-wave loop bound has to carry; 16 x 16 is a single wave."""
    from floodgan import ops
    from floodgan.regions import rank_plane
    for name in ("bernoulli_0.593", "spiral", "flood", "frame_island"):
        lab, want, d, want_depth, want_scene = _oracle_tables(H, W, name)
        roots, R = want["label"], len(want["label"])
        want_area, want_border = np.zeros(H * W, dtype=np.int32), np.zeros(H * W, dtype=np.int32)
        want_area[roots] = want["area"]
        want_border[roots] = (want["y0"] == 0) | (want["x0"] == 0) | (want["y1"] == H - 1) | (want["x1"] == W - 1)
        depth = _placed(d, 0)
        for shift in (0, 1):
            what = (name, shift)
            labels = _placed(lab, shift)
            assert labels.data_ptr() % 16 == (0, 4)[shift]
            area, border = (torch.full((H, W), 77, dtype=torch.int32, device=DEV) for _ in range(2))
            ops.regions_stats(labels, area, border)
            assert np.array_equal(area.cpu().numpy().ravel(), want_area), what
            assert np.array_equal(border.cpu().numpy().ravel(), want_border), what
            got_R, rank = rank_plane(labels)
            assert got_R == R > 0, what
            table = torch.full((R, 8), 77, dtype=torch.int64, device=DEV)
            ops.regions_table(labels, rank, table)
            for j, col in enumerate(RO.COLUMNS):
                assert np.array_equal(table[:, j].cpu().numpy(), want[col]), (what, col)
            got = ops.depth_table(labels, rank, depth, torch.full((R, 3), 77, dtype=torch.int64, device=DEV))
            for j, col in enumerate(("wet_area", "depth_sum_q", "depth_max_q")):
                assert np.array_equal(got[:, j].cpu().numpy(), want_depth[col]), (what, col)
        got = ops.depth_table(None, None, depth, torch.full((1, 3), 77, dtype=torch.int64, device=DEV))
        assert np.array_equal(got.cpu().numpy()[0], want_scene), name
        assert want_scene[2] == 2 ** 30 and 0 < want_scene[0] < H * W                 # capped, and some pixels left out


# ---- refused calls

def test_refused_calls_leave_their_outputs_as_they_were():
    from floodgan import _lib as L, ops
    lib = L.load()
    H, W = 16, 16
    src = _dev(_values(_seeds(H, W, "checkerboard"), "threshold"))
    ints = [torch.full((H, W), 77, dtype=torch.int32, device=DEV) for _ in range(3)]
    near, d2, labels = ints
    floats = [torch.full((H, W), 77.0, device=DEV) for _ in range(3)]
    shore, depth, elev = floats
    table = torch.full((3, 3), 77, dtype=torch.int64, device=DEV)
    nbytes = lib.fg_nearest_seed_scratch_bytes(H, W)
    assert nbytes == H * W * 4 + W * 8 and lib.fg_nearest_seed_scratch_bytes(0, W) == 0
    assert lib.fg_nearest_seed_scratch_bytes(H, 32769) == 0 and lib.fg_nearest_seed_scratch_bytes(32768, 32768) > 0
    scratch = torch.full((nbytes // 8,), 77, dtype=torch.int64, device=DEV)
    st, null = L.stream_handle(), C.c_void_p(0)
    sv, thr, p = ops.sview(src), L.FG_SCALAR_THRESHOLD, L.ptr
    odd = C.c_void_p(near.data_ptr() + 2)
    refused = [
        lib.fg_nearest_seed(sv, H, W, thr, 1, null, p(d2), p(scratch), st),
        lib.fg_nearest_seed(ops.sview(None), H, W, thr, 1, p(near), p(d2), p(scratch), st),
        lib.fg_nearest_seed(sv, H, W, thr, 1, p(near), p(d2), null, st),
        lib.fg_nearest_seed(sv, 0, W, thr, 1, p(near), p(d2), p(scratch), st),
        lib.fg_nearest_seed(sv, H, 32769, thr, 1, p(near), p(d2), p(scratch), st),
        lib.fg_nearest_seed(sv, 32769, W, thr, 1, p(near), p(d2), p(scratch), st),
        lib.fg_nearest_seed(sv, H, W, L.FG_SCALAR_UNIT, 1, p(near), p(d2), p(scratch), st),
        lib.fg_nearest_seed(sv, H, W, thr, 2, p(near), p(d2), p(scratch), st),
        lib.fg_nearest_seed(sv, H, W, thr, 1, odd, p(d2), p(scratch), st),
        lib.fg_nearest_seed(sv, H, W, thr, 1, p(near), p(d2), C.c_void_p(scratch.data_ptr() + 4), st),
        lib.fg_shore(null, H, W, p(shore), st),
        lib.fg_shore(p(src), H, W, null, st),
        lib.fg_shore(p(src), 0, W, p(shore), st),
        lib.fg_shore(p(shore), H, W, p(shore), st),
        lib.fg_flood_depth(p(src), p(elev), null, H, W, p(depth), st),
        lib.fg_flood_depth(p(src), null, p(near), H, W, p(depth), st),
        lib.fg_flood_depth(p(src), p(elev), p(near), H, 0, p(depth), st),
        lib.fg_flood_depth(p(src), p(elev), p(near), 65536, 32768, p(depth), st),
        lib.fg_flood_depth(p(src), p(elev), p(near), H, W, p(elev), st),
        lib.fg_depth_table(p(labels), p(near), null, H, W, p(table), 3, st),
        lib.fg_depth_table(p(labels), null, p(depth), H, W, p(table), 3, st),
        lib.fg_depth_table(p(labels), p(near), p(depth), H, W, p(table), 0, st),
        lib.fg_depth_table(p(labels), p(near), p(depth), H, W, p(table), H * W + 1, st),
        lib.fg_depth_table(null, null, p(depth), H, W, p(table), 3, st),
        lib.fg_depth_table(p(labels), p(near), p(depth), 0, W, p(table), 3, st),
    ]
    assert refused == [-1] * len(refused)                     # FG_ERR_INVALID
    assert b"sizes must be positive" in lib.fg_last_error()
    # the Python wrappers, before the library is called
    with pytest.raises(RuntimeError, match="nearest plane is a contiguous"):
        ops.nearest_seed(src, "threshold", True, torch.full((H, W + 1), 77, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="table is a contiguous int64 \\[R, 3\\]"):
        ops.depth_table(None, None, depth, torch.zeros((1, 8), dtype=torch.int64, device=DEV))
    from floodgan.depth import flood_depth, nearest_seed
    with pytest.raises(ValueError, match="at most 32768"):
        nearest_seed(torch.zeros(1, device=DEV).expand(2, 32769), "threshold")
    with pytest.raises(ValueError, match="the elevation is"):
        flood_depth(src, torch.zeros((H, W + 1), device=DEV))
    with pytest.raises(ValueError, match="on one HIP device"):
        flood_depth(src, torch.zeros((H, W)))
    torch.cuda.synchronize()
    for t in ints + [table, scratch]:
        assert bool((t == 77).all())
    for t in floats:
        assert bool((t == 77.0).all())
    # and the same buffers take an accepted call
    ops.nearest_seed(src, "threshold", True, near, d2)
    _check_planes((near, d2), _oracle(H, W, "checkerboard", True), "accepted")


# ---- predict_scene

class _Identity(torch.nn.Module):
    def forward(self, x):
        return x[:, :3]


def _patch_unet(monkeypatch):
    """predict_scene's U-Net path replaced by a known logit pattern: +4 where the picture's first channel is positive,
    -4 elsewhere.  Blended over the windows (integer weights of at most 8 x 8, nine windows) such a logit is 0 or at
    least 4 / 576 in magnitude, so `> 0` on the host is the device's decision."""
    from floodgan import scene
    monkeypatch.setattr(scene, "_unet", lambda seg_model, batch_stats: seg_model)
    monkeypatch.setattr(scene, "_flood_logits",
                        lambda unet, images, batch_stats: torch.where(images[:, :1] > 0, 4.0, -4.0))


def test_predict_scene_gains_the_depth_keys_only_when_asked(monkeypatch):
    from floodgan.depth import flood_depth
    from floodgan.scene import predict_scene
    _patch_unet(monkeypatch)
    H, W, tile, overlap = 48, 56, 16, 8
    mask = RO.bernoulli(H, W, 0.593, 593)
    x = torch.from_numpy(np.where(mask, 0.5, -0.5).astype(np.float32))[None, None].repeat(1, 3, 1, 1).to(DEV)
    elev_host = _elevation(H, W, False)
    elev = torch.from_numpy(elev_host).to(DEV)
    common = dict(tile=tile, overlap=overlap, batch=5, seg_model="stub")
    plain = predict_scene(_Identity(), x, **common)
    assert set(plain) == {"grid", "output", "flood_logits", "flood_fraction"}                 # the keys before, exactly
    assert np.array_equal(plain["flood_logits"][0, 0].cpu().numpy() > 0, mask)
    assert plain["flood_fraction"] == int(mask.sum()) / (H * W)
    sieved = predict_scene(_Identity(), x, min_region=8, min_hole=8, connectivity=4, **common)
    assert set(sieved) == set(plain) | {"flood_mask", "regions", "flood_fraction_sieved"}
    want = RO.flood_regions(mask, 8, 8, 4)
    assert np.array_equal(sieved["flood_mask"][0, 0].cpu().numpy(), want["mask"].astype(np.float32))
    assert np.array_equal(sieved["regions"]["labels"].cpu().numpy(), want["labels"])
    for minima, form in (({}, elev), (dict(min_region=8, min_hole=8, connectivity=4), elev[None, None])):
        res = predict_scene(_Identity(), x, elevation=form, pixel_area=0.25, **minima, **common)
        assert set(res) == set(plain) | {"flood_mask", "regions", "flood_depth", "depth"} | \
            ({"flood_fraction_sieved"} if minima else set())
        assert torch.equal(res["flood_logits"], plain["flood_logits"]) and torch.equal(res["output"], plain["output"])
        regions = RO.flood_regions(mask, minima.get("min_region", 1), minima.get("min_hole", 0),
                                   minima.get("connectivity", 8))
        assert np.array_equal(res["flood_mask"][0, 0].cpu().numpy(), regions["mask"].astype(np.float32))
        assert np.array_equal(res["regions"]["labels"].cpu().numpy(), regions["labels"])
        assert "mask" not in res["regions"] and "depth" not in res["depth"]
        alone = flood_depth(res["flood_mask"], elev, pixel_area=0.25)
        assert torch.equal(res["flood_depth"], alone["depth"])
        assert torch.equal(res["depth"]["nearest_shore"], alone["nearest_shore"])
        oracle = DO.flood_depth(regions["mask"], elev_host, regions["labels"], regions["table"]["area"], 0.25)
        _same_depth(dict(res["depth"], depth=res["flood_depth"]), oracle, minima)
    with pytest.raises(ValueError, match="needs seg_model"):
        predict_scene(_Identity(), x, tile=tile, overlap=overlap, elevation=elev)
    with pytest.raises(ValueError, match="elevation must be a float32"):
        predict_scene(_Identity(), x, elevation=elev[:, :-1], **common)


def test_model_predict_scene_writes_the_depth_picture_and_the_csv_columns(tmp_path, monkeypatch):
    from floodgan.model import Model
    from floodgan.png import read_png
    _patch_unet(monkeypatch)
    root = str(tmp_path)
    H, W = 40, 56
    raw = np.random.default_rng(21).random((H, W, 9)).astype(np.float32)
    path = os.path.join(root, "harvey_scene.tif")
    write_tiff(path, raw)
    m = Model(model="PairedAttention", training_model=False, data_path=root, resize=None, crop=None,
              train_loader=[], device=DEV)
    common = dict(tile=32, overlap=8, batch=3, seg_model_path="stub")
    before = m.predict_scene(path, **common)
    assert set(before) == {"prediction", "flood_mask", "flood_fraction", "grid"}              # the keys before, exactly
    elev = raw[:, :, 3] * np.float32(100)
    for vmax_arg, minima in ((None, {}), (16.0, dict(min_region=6, min_hole=6, connectivity=4))):
        written = m.predict_scene(path, depth=True, pixel_area=2.0, depth_vmax=vmax_arg, **minima, **common)
        assert set(written) == set(before) | {"regions", "region_count", "flood_depth", "max_depth", "mean_depth",
                                              "volume"}
        assert written["flood_depth"] == f"{root}/images/harvey_scene_floodDepth.png"
        mask = m.last_scene["flood_logits"][0, 0].cpu().numpy() > 0
        regions = RO.flood_regions(mask, minima.get("min_region", 1), minima.get("min_hole", 0),
                                   minima.get("connectivity", 8))
        want = DO.flood_depth(regions["mask"], elev, regions["labels"], regions["table"]["area"], 2.0)
        assert want["max_depth"] > 1 and want["wet_area"] > 0                      # there is depth to draw
        for key in ("max_depth", "mean_depth", "volume"):
            assert written[key] == want[key], key
        vmax = np.float32(vmax_arg if vmax_arg is not None else want["max_depth"])
        unit = np.clip(want["depth"] / vmax, np.float32(0), np.float32(1))
        assert unit.dtype == np.float32 and (vmax_arg is None or unit.max() == 1.0)          # 16 clips this scene
        img, text = read_png(written["flood_depth"])
        assert text == {} and img.tobytes() == PO.scalar_bytes(unit, cmap="gray_r", kind="unit").tobytes()
        lines = open(written["regions"]).read().splitlines()
        assert lines[0].split(",")[10:] == ["wet_area", "mean_depth", "max_depth", "volume"]
        assert lines[0].split(",")[:8] == list(RO.COLUMNS) and len(lines) == regions["count"] + 1
        rows = [line.split(",") for line in lines[1:]]
        assert [int(r[1]) for r in rows] == regions["table"]["area"].tolist()
        assert [int(r[10]) for r in rows] == want["table"]["wet_area"].tolist()
        for j, col in enumerate(("mean_depth", "max_depth", "volume")):
            assert np.array_equal(np.array([float(r[11 + j]) for r in rows]), want["table"][col]), col
    # a scene of no depth at all is drawn over vmax 1; a file without the stack's elevation is refused
    flat = raw.copy()
    flat[:, :, 3] = 0.25
    write_tiff(os.path.join(root, "flat.tif"), flat)
    written = m.predict_scene(os.path.join(root, "flat.tif"), depth=True, **common)
    assert written["max_depth"] == 0.0 and written["volume"] == 0.0
    img, _ = read_png(written["flood_depth"])
    assert img.tobytes() == PO.scalar_bytes(np.zeros((H, W), np.float32), cmap="gray_r", kind="unit").tobytes()
    write_tiff(os.path.join(root, "rgb.tif"), raw[:, :, :3].copy())
    with pytest.raises(ValueError, match="has 3 channels"):
        m.predict_scene(os.path.join(root, "rgb.tif"), depth=True, **common)
    with pytest.raises(ValueError, match="needs seg_model_path"):
        m.predict_scene(path, tile=32, overlap=8, depth=True)
