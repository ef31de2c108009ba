"""The flood regions on the HIP path (csrc/regions.hip through floodgan.regions) against the numpy oracle
(tests/regions_oracle.py).  Everything is an integer or a 0 / 1 float: every comparison is exact equality.

The tile of the labelling kernel is 16 rows x 64 columns: 41 x 53 and 96 x 130 cross row borders, 96 x 130 and
257 x 515 column borders (two and eight of them), and no shape is a multiple of the tile."""
import functools
import os

import numpy as np
import pytest
import torch

import regions_oracle as RO
from tiff_util import write_tiff

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 1), (1, 37), (37, 1), (16, 16), (41, 53), (96, 130)]
BIG = (257, 515)
BIG_PATTERNS = ["flood", "checkerboard", "spiral", "serpentine", "bernoulli_0.593"]
CASES = [(H, W, name) for H, W in SHAPES for name in RO.PATTERNS] + [BIG + (name,) for name in BIG_PATTERNS]
MINIMA = [(1, 0), (8, 0), (8, 8), (1, 1000)]
SPECIALS = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 88.0, -88.0, float("inf"), float("-inf"), float("nan")]


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
def _oracle_labels(H, W, name, target, connectivity):
    out = RO.label_class(_mask(H, W, name), target, connectivity)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_regions(H, W, name, min_region, min_hole, connectivity):
    return RO.flood_regions(_mask(H, W, name), min_region, min_hole, connectivity)


def _plane(mask):
    """the mask as a contiguous fp32 [1, 1, H, W] device tensor of 0 / 1 (kind "threshold")"""
    return torch.from_numpy(mask.astype(np.float32))[None, None].to(DEV)


def _shape_cases(H, W):
    return [name for h, w, name in CASES if (h, w) == (H, W)]


def _same_table(got, want, what):
    assert set(got) == set(RO.COLUMNS), what
    for col in RO.COLUMNS:
        assert got[col].dtype == np.int64 and np.array_equal(got[col], want[col]), (what, col)


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("H,W", SHAPES + [BIG])
def test_label_regions_equals_the_oracle(H, W, connectivity):
    from floodgan.regions import label_regions
    for name in _shape_cases(H, W):
        src = _plane(_mask(H, W, name))
        for target in (True, False):
            got = label_regions(src, "threshold", target, connectivity)
            assert got.dtype == torch.int32 and tuple(got.shape) == (H, W) and got.is_cuda
            want = _oracle_labels(H, W, name, target, connectivity)
            assert np.array_equal(got.cpu().numpy(), want), (name, target)
    if (H, W) == (96, 130):
        cb = label_regions(_plane(_mask(H, W, "checkerboard")), "threshold", True, connectivity)
        roots = int((cb.view(-1) == torch.arange(H * W, device=DEV, dtype=torch.int32)).sum())
        assert roots == (1 if connectivity == 8 else H * W // 2)


@pytest.mark.parametrize("min_region,min_hole", MINIMA)
@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("H,W", SHAPES + [BIG])
def test_sieve_and_table_equal_the_oracle(H, W, connectivity, min_region, min_hole):
    from floodgan.regions import flood_regions
    for name in _shape_cases(H, W):
        want = _oracle_regions(H, W, name, min_region, min_hole, connectivity)
        got = flood_regions(_plane(_mask(H, W, name)), "threshold", min_region, min_hole, connectivity)
        what = (name, H, W, connectivity, min_region, min_hole)
        mask = got["mask"]
        assert mask.dtype == torch.float32 and tuple(mask.shape) == (1, 1, H, W), what
        assert np.array_equal(mask[0, 0].cpu().numpy(), want["mask"].astype(np.float32)), what
        assert (got["removed"], got["filled"]) == (want["removed"], want["filled"]), what
        assert np.array_equal(got["labels"].cpu().numpy(), want["labels"]) and got["labels"].dtype == torch.int32, what
        assert got["count"] == want["count"] == len(got["table"]["label"]), what
        _same_table(got["table"], want["table"], what)
        assert got["centroids"].dtype == np.float64 and got["centroids"].shape == (want["count"], 2), what
        assert np.array_equal(got["centroids"], want["centroids"]), what
        assert got["flood_fraction"] == want["flood_fraction"], what
    if (H, W) == (96, 130) and (min_region, min_hole) == (8, 8):
        busy = _oracle_regions(H, W, "bernoulli_0.593", 8, 8, 4)
        assert busy["removed"] > 100 and busy["filled"] > 50              # the sieve has work to do at this shape


def test_table_false_skips_the_table_and_keeps_the_rest():
    from floodgan.regions import flood_regions
    H, W, name = 41, 53, "bernoulli_0.5"
    want = _oracle_regions(H, W, name, 8, 8, 8)
    got = flood_regions(_plane(_mask(H, W, name)), "threshold", 8, 8, 8, table=False)
    assert got["table"] is None and got["centroids"] is None and got["count"] == want["count"]
    assert np.array_equal(got["labels"].cpu().numpy(), want["labels"])
    assert (got["removed"], got["filled"], got["flood_fraction"]) == (want["removed"], want["filled"],
                                                                      want["flood_fraction"])


def _forms(values):
    """a float32 [H, W] numpy plane in the three forms the kernels read"""
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
def test_every_input_form_and_kind_gives_the_same_regions(kind):
    from floodgan.regions import flood_regions, label_regions
    H, W, name = 41, 53, "bernoulli_0.593"
    mask = _mask(H, W, name)
    rng = np.random.default_rng(11)
    if kind == "threshold":
        values = np.where(mask, rng.uniform(0.51, 2.0, (H, W)), rng.uniform(-2.0, 0.5, (H, W))).astype(np.float32)
    else:
        values = np.where(mask, rng.uniform(0.01, 9.0, (H, W)), rng.uniform(-9.0, -0.01, (H, W))).astype(np.float32)
    want = _oracle_regions(H, W, name, 8, 8, 8)
    for form, src in _forms(values).items():
        got = flood_regions(src, kind, 8, 8, 8)
        assert np.array_equal(got["labels"].cpu().numpy(), want["labels"]), form
        _same_table(got["table"], want["table"], form)
        lab = label_regions(src, kind, False, 4)
        assert np.array_equal(lab.cpu().numpy(), _oracle_labels(H, W, name, False, 4)), form


def test_special_values_decide_as_fg_mask_confusion_does():
    from floodgan import ops
    from floodgan.regions import flood_regions
    H, W = 41, 53
    values = np.resize(np.array(SPECIALS, dtype=np.float32), (H, W))
    z = torch.from_numpy(values)[None, None].to(DEV).contiguous()
    counted = int(ops.flood_count(z).cpu())
    got = flood_regions(z, "logit", 1, 0, 8)
    assert round(got["flood_fraction"] * H * W) == counted and int(got["mask"].sum()) == counted
    # +0, -0, NaN, the negatives and -inf are dry; 2^-20, 88 and +inf are flood
    want = np.isin(np.arange(H * W) % len(SPECIALS), [2, 4, 6]).reshape(H, W)
    assert np.array_equal(got["mask"][0, 0].cpu().numpy() > 0, want)
    assert np.array_equal(got["labels"].cpu().numpy(), RO.label(want, 8))
    # kind "threshold": x > 0.5 (NaN is not)
    thr = flood_regions(z, "threshold", 1, 0, 8)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(thr["mask"][0, 0].cpu().numpy() > 0, values > 0.5)


def test_two_calls_are_bit_identical_and_the_transpose_follows_its_oracle():
    from floodgan.regions import flood_regions
    H, W, name = 96, 130, "bernoulli_0.593"
    mask = _mask(H, W, name)
    src = _plane(mask)
    a, b = (flood_regions(src, "threshold", 8, 8, 4) for _ in range(2))
    assert torch.equal(a["labels"], b["labels"]) and torch.equal(a["mask"], b["mask"])
    for col in RO.COLUMNS:
        assert a["table"][col].tobytes() == b["table"][col].tobytes(), col
    want = RO.flood_regions(np.ascontiguousarray(mask.T), 8, 8, 4)
    got = flood_regions(_plane(np.ascontiguousarray(mask.T)), "threshold", 8, 8, 4)
    assert np.array_equal(got["labels"].cpu().numpy(), want["labels"])
    _same_table(got["table"], want["table"], "transpose")
    # the transposed VIEW of the same memory (row stride 1, column stride W) reads the same scene
    view = flood_regions(src[0, 0].t()[None, None], "threshold", 8, 8, 4)
    assert torch.equal(view["labels"], got["labels"])


def test_refused_calls_leave_their_outputs_as_they_were():
    import ctypes as C

    from floodgan import _lib as L, ops
    lib = L.load()
    H, W = 16, 16
    src = _plane(_mask(H, W, "checkerboard"))
    labels = torch.full((H, W), 77, dtype=torch.int32, device=DEV)
    planes = [torch.full((H, W), 77, dtype=torch.int32, device=DEV) for _ in range(2)]
    mask = torch.full((1, 1, H, W), 77.0, device=DEV)
    counts = torch.full((2,), 77, dtype=torch.int64, device=DEV)
    table = torch.full((3, 8), 77, dtype=torch.int64, device=DEV)
    st, null = L.stream_handle(), C.c_void_p(0)
    sv = ops.sview(src)
    thr = L.FG_SCALAR_THRESHOLD
    refused = [
        lib.fg_regions_label(sv, H, W, thr, 1, 8, null, st),
        lib.fg_regions_label(ops.sview(None), H, W, thr, 1, 8, L.ptr(labels), st),
        lib.fg_regions_label(sv, H, W, thr, 1, 6, L.ptr(labels), st),
        lib.fg_regions_label(sv, H, W, L.FG_SCALAR_UNIT, 1, 8, L.ptr(labels), st),
        lib.fg_regions_label(sv, H, W, thr, 2, 8, L.ptr(labels), st),
        lib.fg_regions_label(sv, 65536, 32768, thr, 1, 8, L.ptr(labels), st),
        lib.fg_regions_label(sv, 0, W, thr, 1, 8, L.ptr(labels), st),
        lib.fg_regions_stats(L.ptr(labels), H, W, null, L.ptr(planes[1]), st),
        lib.fg_regions_stats(L.ptr(labels), 65536, 32768, L.ptr(planes[0]), L.ptr(planes[1]), st),
        lib.fg_regions_table(L.ptr(labels), null, H, W, L.ptr(table), 3, st),
        lib.fg_regions_table(L.ptr(labels), L.ptr(planes[0]), H, W, L.ptr(table), 0, st),
        lib.fg_regions_apply(L.ptr(labels), null, null, H, W, L.FG_REGIONS_REMOVE, 8, L.ptr(mask), L.ptr(counts), st),
        lib.fg_regions_apply(L.ptr(labels), L.ptr(planes[0]), null, H, W, L.FG_REGIONS_FILL, 8, L.ptr(mask),
                             L.ptr(counts), st),
        lib.fg_regions_apply(L.ptr(labels), L.ptr(planes[0]), L.ptr(planes[1]), H, W, 2, 8, L.ptr(mask), L.ptr(counts),
                             st),
        lib.fg_regions_apply(L.ptr(labels), L.ptr(planes[0]), L.ptr(planes[1]), H, W, L.FG_REGIONS_FILL, -1,
                             L.ptr(mask), L.ptr(counts), st),
    ]
    assert refused == [-1] * len(refused)                     # FG_ERR_INVALID
    assert b"min_area -1" in lib.fg_last_error()
    # the Python wrapper: a labels buffer of the wrong size, before the library is called
    with pytest.raises(RuntimeError, match="labels plane is a contiguous"):
        ops.regions_label(src, "threshold", True, 8, torch.full((H, W + 1), 77, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="labels plane is a contiguous"):
        ops.regions_label(src, "threshold", True, 8, torch.full((H, W), 77, dtype=torch.int64, device=DEV))
    from floodgan.regions import label_regions
    with pytest.raises(ValueError, match="below 2\\^31"):
        label_regions(torch.zeros(1, device=DEV).expand(65536, 32768))
    torch.cuda.synchronize()
    for t in [labels, counts, table] + planes:
        assert bool((t == 77).all())
    assert bool((mask == 77.0).all())
    # and the same buffers take an accepted call
    ops.regions_label(src, "threshold", True, 8, labels)
    assert np.array_equal(labels.cpu().numpy(), _oracle_labels(H, W, "checkerboard", True, 8))


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


def test_predict_scene_gains_the_region_keys_only_when_asked(monkeypatch):
    from floodgan.scene import predict_scene
    _patch_unet(monkeypatch)
    H, W, tile, overlap = 48, 56, 16, 8
    mask = RO.bernoulli(H, W, 0.593, 593)
    x = torch.from_numpy(np.where(mask, 0.5, -0.5).astype(np.float32))[None, None].repeat(1, 3, 1, 1).to(DEV)
    plain = predict_scene(_Identity(), x, tile=tile, overlap=overlap, batch=5, seg_model="stub")
    assert set(plain) == {"grid", "output", "flood_logits", "flood_fraction"}                 # today's keys, exactly
    assert np.array_equal(plain["flood_logits"][0, 0].cpu().numpy() > 0, mask)
    for min_region, min_hole, connectivity in [(8, 8, 4), (8, None, 8), (None, 1000, 8)]:
        res = predict_scene(_Identity(), x, tile=tile, overlap=overlap, batch=5, seg_model="stub",
                            min_region=min_region, min_hole=min_hole, connectivity=connectivity)
        assert set(res) == set(plain) | {"flood_mask", "regions", "flood_fraction_sieved"}
        assert torch.equal(res["flood_logits"], plain["flood_logits"])
        assert res["flood_fraction"] == plain["flood_fraction"] == int(mask.sum()) / (H * W)
        want = RO.flood_regions(mask, min_region or 1, min_hole or 0, connectivity)
        assert np.array_equal(res["flood_mask"][0, 0].cpu().numpy(), want["mask"].astype(np.float32))
        reg = res["regions"]
        assert set(reg) == {"labels", "count", "table", "centroids", "removed", "filled", "flood_fraction"}
        assert np.array_equal(reg["labels"].cpu().numpy(), want["labels"]) and reg["count"] == want["count"]
        _same_table(reg["table"], want["table"], (min_region, min_hole))
        assert (reg["removed"], reg["filled"]) == (want["removed"], want["filled"])
        assert res["flood_fraction_sieved"] == want["flood_fraction"] == reg["flood_fraction"]
    with pytest.raises(ValueError, match="need seg_model"):
        predict_scene(_Identity(), x, tile=tile, overlap=overlap, min_region=8)
    with pytest.raises(ValueError, match="connectivity 6"):
        predict_scene(_Identity(), x, tile=tile, overlap=overlap, seg_model="stub", min_hole=2, connectivity=6)


def test_model_predict_scene_writes_the_sieved_mask_and_the_csv(tmp_path, monkeypatch):
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
    before = m.predict_scene(path, tile=32, overlap=8, batch=3, seg_model_path="stub")
    assert set(before) == {"prediction", "flood_mask", "flood_fraction", "grid"}              # today's keys, exactly
    unsieved = read_png(before["flood_mask"])[0]
    written = m.predict_scene(path, tile=32, overlap=8, batch=3, seg_model_path="stub", min_region=6, min_hole=6,
                              connectivity=4)
    assert set(written) == set(before) | {"regions", "region_count"}
    assert written["flood_mask"] == f"{root}/images/harvey_scene_floodMask.png"
    assert written["regions"] == f"{root}/images/harvey_scene_floodRegions.csv"
    logits = m.last_scene["flood_logits"][0, 0].cpu().numpy()
    assert np.abs(logits[logits != 0]).min() >= 4 / 576
    mask = logits > 0
    assert np.array_equal(unsieved[..., 0] == 255, mask)
    want = RO.flood_regions(mask, 6, 6, 4)
    assert want["removed"] + want["filled"] > 0                               # the sieve changed this scene
    img, text = read_png(written["flood_mask"])
    assert img.shape == (H, W, 4) and text == {} and set(np.unique(img[..., 0])) <= {0, 255}
    assert np.array_equal(img[..., 0] == 255, want["mask"]) and (img[..., 3] == 255).all()
    assert written["region_count"] == want["count"] and written["flood_fraction"] == int(mask.sum()) / (H * W)
    lines = open(written["regions"]).read().splitlines()
    assert lines[0].split(",")[:8] == list(RO.COLUMNS) and len(lines) == want["count"] + 1
    rows = np.array([[int(v) for v in line.split(",")[:8]] for line in lines[1:]], dtype=np.int64).reshape(-1, 8)
    for j, col in enumerate(RO.COLUMNS):
        assert np.array_equal(rows[:, j], want["table"][col]), col
