"""Whole scenes on the HIP path: fg_mosaic_accumulate / fg_mosaic_finalize against the numpy fp64 oracle of the blend
(tests/scene_oracle.py), and predict_scene / Model.predict_scene on top of them.

The blend's tolerance is derived, not measured: a pixel sees at most nine fp32 products and nine fp32 adds of values
|v| <= 1 with exact integer weights, then one division by the exact weight sum -- each operation within 2^-24
relative of a partial result that never exceeds the weight sum -- so the blended value is within 19 * 2^-24 < 1.2e-6
of the exact one; the tests allow 2e-6 (times max |v| for logits, whose magnitude is not 1)."""
import functools
import os

import numpy as np
import pytest
import torch

import scene_oracle as SO
from test_gpu_parity import DEV
from tiff_util import write_tiff

pytestmark = pytest.mark.gpu

TOL = 2e-6
# (H, W, tile, overlap): 1x1 grid; last window shifted by one; odd sizes and scalar tails (twice); triple coverage,
# nine windows on some pixels; no overlap, the shifted window averaged
GEOMETRIES = [(16, 16, 16, 8), (17, 16, 16, 8), (41, 53, 16, 8), (41, 53, 16, 4), (72, 40, 32, 16), (33, 48, 16, 0)]
LAYOUTS = ["nchw", "channels_last", "buf"]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@functools.lru_cache(maxsize=None)
def _case(H, W, tile, overlap, c):
    """(windows float32 [K, c, tile, tile] in [-1, 1], their fp64 oracle blend [c, H, W]); computed once, read-only"""
    k = len(SO.starts(H, tile, overlap)) * len(SO.starts(W, tile, overlap))
    rng = np.random.default_rng(1000 * H + 10 * W + tile + overlap + c)
    wins = rng.uniform(-1, 1, (k, c, tile, tile)).astype(np.float32)
    want = SO.blend(wins, H, W, tile, overlap)
    wins.setflags(write=False)
    want.setflags(write=False)
    return wins, want


def _source(layout, wins):
    """the windows on the device in one of the layouts the kernels read"""
    from floodgan.plans import Buf
    k, c, tile, _ = wins.shape
    t = torch.from_numpy(wins.copy()).to(DEV)
    if layout == "nchw":
        return t
    if layout == "channels_last":                       # channels 0 .. c - 1 of a wider channels-last tensor
        wide = torch.full((k, c + 2, tile, tile), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)
        wide[:, :c] = t
        assert wide.stride(3) == c + 2 and wide.stride(1) == 1
        return wide
    buf = Buf.empty(k, tile, tile, 4, 0, DEV)           # channels 0 .. c - 1 of a 4-channel NHWC Buf (the logits' form)
    buf.t.fill_(7.0)
    buf.interior()[..., :c] = t.permute(0, 2, 3, 1)
    return buf


def _slice(src, k0, n):
    from floodgan.plans import Buf
    if isinstance(src, Buf):
        return Buf(src.t[k0 * src.s_img:(k0 + n) * src.s_img], n, src.h, src.w, src.c, src.pad)
    return src[k0:k0 + n]


def _blend(src, H, W, c, tile, overlap, batch):
    from floodgan.scene import Mosaic
    mo = Mosaic(H, W, c, tile, overlap, DEV)
    for k0, n in mo.batches(batch):
        mo.add(_slice(src, k0, n), k0)
    return mo.result(), mo


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("H,W,tile,overlap", GEOMETRIES)
def test_mosaic_matches_the_oracle(H, W, tile, overlap, c, layout):
    wins, want = _case(H, W, tile, overlap, c)
    got, mo = _blend(_source(layout, wins), H, W, c, tile, overlap, wins.shape[0])
    assert mo.grid == (SO.starts(H, tile, overlap), SO.starts(W, tile, overlap))
    assert tuple(got.shape) == (1, c, H, W) and got.is_contiguous() and got.dtype == torch.float32
    err = float(np.abs(got[0].cpu().numpy().astype(np.float64) - want).max())
    print(f"mosaic {H}x{W} tile {tile} overlap {overlap} c {c} {layout}: max abs err {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("c,layout", [(3, "channels_last"), (1, "buf"), (3, "nchw")])
def test_batch_split_is_bit_identical(c, layout):
    H, W, tile, overlap = 41, 53, 16, 8
    wins, _ = _case(H, W, tile, overlap, c)
    src = _source(layout, wins)
    whole, mo = _blend(src, H, W, c, tile, overlap, wins.shape[0])
    assert mo.count == 30 and len(mo.xs) == 6
    # 1 and 3 (spans inside a grid row), 4 and 7 (spans that cross grid rows), all at once
    for batch in (1, 3, 4, 7):
        part, mp = _blend(src, H, W, c, tile, overlap, batch)
        assert torch.equal(mp.planes, mo.planes), batch
        assert torch.equal(part, whole), batch


def test_mosaic_refuses_out_of_order_batches():
    from floodgan.scene import Mosaic
    wins, _ = _case(17, 16, 16, 8, 3)
    src = _source("nchw", wins)
    mo = Mosaic(17, 16, 3, 16, 8, DEV)
    with pytest.raises(ValueError, match="ascending order"):
        mo.add(src[1:2], 1)
    with pytest.raises(RuntimeError, match="0 of 2"):
        mo.result()
    mo.add(src[:1], 0)
    with pytest.raises(ValueError, match="ascending order"):
        mo.add(src[:1], 0)
    with pytest.raises(RuntimeError, match="need \\[n, >= 3, 16, 16\\]"):
        mo.add(src[1:2, :, :8], 1)
    mo.add(src[1:2], 1)
    assert tuple(mo.result().shape) == (1, 3, 17, 16)


FILL = 0.625


def _raw_args(H=41, W=53, tile=16, overlap=8, c=3):
    """a valid raw call's pieces: (dict of arguments, keep-alive)"""
    ys, xs = (np.asarray(SO.starts(L, tile, overlap), dtype=np.int32) for L in (H, W))
    yd, xd = torch.from_numpy(ys).to(DEV), torch.from_numpy(xs).to(DEV)
    n = len(ys) * len(xs)
    src = torch.rand(n, c, tile, tile, device=DEV) * 0.5 + 0.5          # positive: every sum moves its plane
    a = dict(src=src.data_ptr(), n=n, c=c, k0=0, H=H, W=W, tile=tile, overlap=overlap, ny=len(ys), nx=len(xs),
             ys=yd.data_ptr(), xs=xd.data_ptr(), ys_host=ys.ctypes.data, xs_host=xs.ctypes.data)
    return a, (ys, xs, yd, xd, src)


def _raw(which, a, planes, dst):
    from floodgan import _lib as L
    g = L.fg_mosaic_grid(a["ys"], a["xs"], a["ys_host"], a["xs_host"], a["ny"], a["nx"], a["tile"], a["overlap"])
    if which == "accumulate":
        t = a["tile"]
        sv = L.fg_sview(a["src"], a["c"] * t * t, t * t, t, 1)
        return L.load().fg_mosaic_accumulate(sv, a["n"], a["c"], g, a["k0"], planes, a["H"], a["W"], L.stream_handle())
    return L.load().fg_mosaic_finalize(planes, a["c"], g, a["H"], a["W"], dst, L.stream_handle())


@pytest.mark.parametrize("which", ["accumulate", "finalize"])
def test_invalid_calls_fail_and_leave_the_planes_untouched(which):
    from floodgan import _lib as L
    from floodgan import ops
    good, keep = _raw_args()
    H, W, c = good["H"], good["W"], good["c"]
    planes = torch.full((c, H, W), FILL, device=DEV)
    dst = torch.full((1, c, H, W), FILL, device=DEV)

    def moved(axis, index, by):
        s = keep[0 if axis == "ys" else 1].copy()
        s[index] += by
        keep_alive.append(s)
        return {axis + "_host": s.ctypes.data}

    keep_alive = []
    bad = [dict(ys=None), dict(xs=None), dict(ys_host=None), dict(xs_host=None),
           dict(H=0), dict(W=-5), dict(tile=0), dict(ny=0), dict(nx=-1),
           dict(c=2), dict(c=0), dict(c=4),
           dict(overlap=-1), dict(overlap=9), dict(tile=2060, overlap=1025),
           dict(tile=48),                                      # larger than the scene
           moved("ys", -1, 1), moved("xs", -1, 1),             # the last window leaves the scene
           moved("ys", 0, -1), moved("xs", 0, 1),              # the first one does / leaves column 0 uncovered
           moved("ys", 2, -8),                                 # starts that do not ascend
           dict(H=H + 1), dict(W=W - 1)]                       # a scene the starts were not made for
    if which == "accumulate":
        bad += [dict(src=None), dict(n=0), dict(n=-2), dict(k0=-1), dict(k0=1), dict(n=good["n"] + 1),
                dict(k0=good["n"], n=1)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        rc = _raw(which, a, planes.data_ptr(), dst.data_ptr())
        assert rc == -1, kw
        assert L.load().fg_last_error().decode().startswith(f"fg_mosaic_{which}"), kw
    assert _raw(which, good, None, dst.data_ptr()) == -1
    if which == "finalize":
        assert _raw(which, good, planes.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert bool((planes == FILL).all()) and bool((dst == FILL).all())
    # the valid call succeeds and writes
    assert _raw(which, good, planes.data_ptr(), dst.data_ptr()) == 0
    torch.cuda.synchronize()
    if which == "accumulate":
        assert bool((planes > FILL).all()) and bool((dst == FILL).all())
    else:
        # pixel (20, 20): rows 8 and 16 cover it with w(12) + w(4) = 4 + 5, and so do columns 8 and 16
        want = torch.tensor(FILL, dtype=torch.float32) / torch.tensor(81.0, dtype=torch.float32)
        assert bool((planes == FILL).all()) and bool((dst[0, :, 20, 20].cpu() == want).all())
        assert bool((dst[0, :, 0, 0] == FILL).all())             # a corner pixel's weight sum is 1
    # and the Python layer raises the library's message
    from floodgan.scene import Mosaic
    mo = Mosaic(H, W, c, good["tile"], good["overlap"], DEV)
    with pytest.raises(RuntimeError, match="fg_mosaic_accumulate: windows 29 .. 30"):
        ops.mosaic_accumulate(keep[4][:2], 29, mo.grid_struct, mo.planes)
    assert bool((mo.planes == 0).all())


# ------------------------------------------------------------------------------------------ predict_scene

class _Identity(torch.nn.Module):
    """a "generator" that returns the scene's RGB channels"""

    def forward(self, x):
        return x[:, :3]


def _scene(H, W, C=9, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((1, C, H, W), generator=g) * 2 - 1).to(DEV)


def _recorded(module):
    """the outputs `module` produces from here on, as host arrays in call order"""
    outs = []
    handle = module.register_forward_hook(lambda m, i, o: outs.append(o.detach().float().cpu().numpy().copy()))
    return outs, handle


def test_predict_scene_identity_generator_returns_the_scene():
    from floodgan.scene import predict_scene
    x = _scene(41, 53)
    gen = _Identity()
    outs, handle = _recorded(gen)
    res = predict_scene(gen, x, tile=16, overlap=8, batch=8)
    handle.remove()
    assert res["grid"] == (SO.starts(41, 16, 8), SO.starts(53, 16, 8)) and set(res) == {"grid", "output"}
    assert [o.shape[0] for o in outs] == [8, 8, 8, 6]                   # the last batch is smaller
    out = res["output"]
    assert tuple(out.shape) == (1, 3, 41, 53) and out.dtype == torch.float32
    err = float((out - x[:, :3]).abs().max())
    print(f"identity generator: max abs err {err:.3e}")
    assert err <= TOL


def _generator(seed=3):
    from floodgan.model import Model
    from floodgan.model_architectures import PairedAttentionGenerator
    torch.manual_seed(seed)
    return PairedAttentionGenerator(input_channels=9).apply(Model.initialise_weights).to(DEV)


def test_predict_scene_real_generator_blends_what_the_generator_produced():
    from floodgan.scene import predict_scene
    H, W, tile, overlap = 72, 88, 32, 8
    gen = _generator()
    x = _scene(H, W)
    outs, handle = _recorded(gen)
    res = predict_scene(gen, x, tile=tile, overlap=overlap, batch=3)
    handle.remove()
    assert [o.shape for o in outs] == [(3, 3, tile, tile)] * 4
    want = SO.blend(np.concatenate(outs), H, W, tile, overlap)
    got = res["output"][0].cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    print(f"PairedAttention scene {H}x{W}: max abs err vs the blend of the recorded outputs {err:.3e}")
    assert np.abs(np.concatenate(outs)).max() <= 1.0 and err <= TOL
    assert gen.training                                                  # the generator ran in the mode it was in


def test_predict_scene_one_window_is_the_generator_output():
    from floodgan.scene import predict_scene
    gen = _generator()
    x = _scene(32, 32)
    torch.manual_seed(47)
    with torch.no_grad():
        direct = gen(x)
    for tile in (32, None):
        res = predict_scene(gen, x, tile=tile, overlap=8, batch=3)
        assert res["grid"] == ([0], [0]) and torch.equal(res["output"], direct), tile


def _unet(seed=9):
    """seeded initialise_weights, the running statistics moved away from (0, 1) so that the two modes differ"""
    from floodgan.segmentation import UNet, initialise_weights
    torch.manual_seed(seed)
    net = UNet().apply(initialise_weights)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, b in net.named_buffers():
            if k.endswith("running_mean"):
                b.add_(torch.randn(b.shape, generator=g) * 0.05)
            elif k.endswith("running_var"):
                b.mul_(0.5 + torch.rand(b.shape, generator=g))
    return net.to(DEV)


@pytest.fixture(scope="module")
def unet():
    return _unet()


def _host_flood_fraction(logits):
    """(lowest, highest) share of flood pixels the decision sigmoid(z) > 0.5 allows: equal unless a logit lies in the
    band |z| <= 2^-21, where an fp32 sigmoid may or may not round to exactly 0.5 (tests/render_oracle.py)"""
    z = logits.detach().cpu().flatten()
    band = z.abs() <= 2.0 ** -21
    sure = int(((torch.sigmoid(z) > 0.5) & ~band).sum())
    return sure / z.numel(), (sure + int(band.sum())) / z.numel()


@pytest.mark.parametrize("batch_stats", [False, True])
def test_predict_scene_with_a_unet(unet, batch_stats, monkeypatch):
    from floodgan import segmentation
    from floodgan.scene import predict_scene
    H, W, tile, overlap = 40, 56, 32, 8
    x = _scene(H, W, seed=6)
    before = {k: v.detach().clone() for k, v in unet.state_dict().items()}
    recorded, modes = [], []
    real = segmentation.unet_logits

    def recording(P, B, X0, training=True, save=False, update_running=True):
        out = real(P, B, X0, training, save, update_running)
        recorded.append(out.interior()[..., :1].permute(0, 3, 1, 2).cpu().numpy().copy())
        modes.append((training, save, update_running))
        return out

    monkeypatch.setattr(segmentation, "unet_logits", recording)
    res = predict_scene(_Identity(), x, tile=tile, overlap=overlap, batch=3, seg_model=unet, batch_stats=batch_stats)
    assert modes == [(batch_stats, False, False)] * 2 and [r.shape[0] for r in recorded] == [3, 1]
    wins = np.concatenate(recorded)
    want = SO.blend(wins, H, W, tile, overlap)
    logits = res["flood_logits"]
    assert tuple(logits.shape) == (1, 1, H, W) and logits.dtype == torch.float32
    scale = float(np.abs(wins).max())
    err = float(np.abs(logits[0].cpu().numpy().astype(np.float64) - want).max())
    print(f"U-Net scene batch_stats={batch_stats}: max |logit| {scale:.3e}, max abs err {err:.3e}")
    assert scale > 0 and err <= TOL * scale
    lo, hi = _host_flood_fraction(logits)
    assert isinstance(res["flood_fraction"], float) and lo <= res["flood_fraction"] <= hi
    after = unet.state_dict()
    assert set(after) == set(before) and any(k.endswith("num_batches_tracked") for k in before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def test_predict_scene_two_modes_differ_and_bad_tiles_raise(unet):
    from floodgan.scene import predict_scene
    x = _scene(40, 56, seed=6)
    with pytest.raises(ValueError, match="tile must be a multiple of 16 \\(got 24\\)"):
        predict_scene(_Identity(), x, tile=24, overlap=8, seg_model=unet)
    with pytest.raises(ValueError, match="H must be a multiple of 16 \\(got 40\\)"):
        predict_scene(_Identity(), x, tile=None, seg_model=unet)
    with pytest.raises(ValueError, match="tile 64"):
        predict_scene(_Identity(), x, tile=64, overlap=8)
    with pytest.raises(TypeError, match="FloodMaskLoss takes"):
        predict_scene(_Identity(), x, tile=32, overlap=8, seg_model=torch.nn.Identity())
    with pytest.raises(ValueError, match="overlap 64"):                  # the default overlap is for tiles of 128 up
        predict_scene(_Identity(), x, tile=32, seg_model=unet)
    a = predict_scene(_Identity(), x[..., :32, :32], tile=32, overlap=8, seg_model=unet, batch_stats=False)
    b = predict_scene(_Identity(), x[..., :32, :32], tile=None, seg_model=unet, batch_stats=True)
    assert tuple(a["flood_logits"].shape) == (1, 1, 32, 32) and not torch.equal(a["flood_logits"], b["flood_logits"])
    lo, hi = _host_flood_fraction(a["flood_logits"])
    assert lo <= a["flood_fraction"] <= hi


def test_model_predict_scene(tmp_path, unet):
    from floodgan.data import load_scene
    from floodgan.model import Model
    from floodgan.png import read_png
    from floodgan.render import save_image
    root = str(tmp_path)
    H, W = 40, 56
    raw = np.random.default_rng(21).random((H, W, 9)).astype(np.float32)
    path = os.path.join(root, "harvey_scene.tif")
    write_tiff(path, raw)
    x = load_scene(path, "all", DEV)
    assert tuple(x.shape) == (1, 9, H, W)
    assert float((x.cpu() - torch.from_numpy(raw).permute(2, 0, 1)[None].sub(0.5).div(0.5)).abs().max()) <= 1e-6
    dem = load_scene(path, "dem", DEV)
    assert torch.equal(dem, x[:, [0, 1, 2, 3]])
    m = Model(model="PairedAttention", training_model=False, data_path=root, resize=None, crop=None,
              train_loader=[], device=DEV)
    with pytest.raises(ValueError, match="tile 512"):
        m.predict_scene(path)                                           # the model's own size: larger than this scene
    written = m.predict_scene(path, tile=32, overlap=8, batch=3, seg_model_path=unet)
    assert written["prediction"] == f"{root}/images/harvey_scene_prediction.png"
    assert written["flood_mask"] == f"{root}/images/harvey_scene_floodMask.png"
    assert written["grid"] == (SO.starts(H, 32, 8), SO.starts(W, 32, 8))
    res = m.last_scene
    for key, tensor, kind in (("prediction", res["output"], "rgb"), ("flood_mask", res["flood_logits"], "mask_logits")):
        img, text = read_png(written[key])
        assert img.shape == (H, W, 4) and text == {}
        again = save_image(os.path.join(root, f"{key}_again.png"), tensor, kind)
        assert open(again, "rb").read() == open(written[key], "rb").read(), key
    lo, hi = _host_flood_fraction(res["flood_logits"])
    assert written["flood_fraction"] == res["flood_fraction"] and lo <= written["flood_fraction"] <= hi
    # without a segmentation model: the prediction only, into a directory of the caller's
    other = m.predict_scene(path, tile=32, overlap=8, out_dir=os.path.join(root, "elsewhere"))
    assert other["prediction"] == f"{root}/elsewhere/harvey_scene_prediction.png" and os.path.exists(other["prediction"])
    assert other["flood_mask"] is None and other["flood_fraction"] is None
    assert open(other["prediction"], "rb").read() == open(written["prediction"], "rb").read()
