"""Pictures on the HIP path: fg_render_rgb / fg_render_scalar against the numpy oracle of the imsave byte rules
(tests/render_oracle.py, pinned to matplotlib by tests/test_render_cpu.py) -- every byte, every byte around the
panels -- and the reference's plotting methods on top of them."""
import json
import os

import numpy as np
import pytest
import torch

import render_oracle as RO
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu

FILL = 0x5A
GEOMETRIES = [(1, 1, 1), (1, 3, 5), (2, 7, 67), (1, 16, 64), (3, 5, 130)]
SOURCES = ["nchw3", "nchw9", "channels_last9", "w_sliced"]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _values(pool, size, rng):
    """`size` values drawn from pool, every pool value present when size allows"""
    flat = pool[rng.integers(len(pool), size=size)]
    k = min(len(pool), size)
    flat[rng.permutation(size)[:k]] = pool[rng.permutation(len(pool))[:k]]
    return flat


def _source(kind, values, n, h, w):
    """(device view [n, >= 3, h, w], host float32 [n, C, h, w] of what the view shows)"""
    c = 3 if kind in ("nchw3", "w_sliced") else 9
    wide = w + 5 if kind == "w_sliced" else w
    host = torch.from_numpy(values[:n * c * h * wide].reshape(n, c, h, wide).copy())
    dev = host.to(DEV)
    if kind == "channels_last9":
        dev = dev.contiguous(memory_format=torch.channels_last)
        if n * h * w > 1:
            assert dev.stride(3) == c
    if kind == "w_sliced":
        host, dev = host[..., 2:2 + w], dev[..., 2:2 + w]
        assert not dev.is_contiguous() or w == 1
    return dev, host.numpy()


PLACEMENTS = [(row0, col0, aligned, down) for row0 in (0, 2) for col0 in (0, 1, 3, 4) for aligned in (True, False)
              for down in (True, False)]


def _canvas(n, h, w, row0, col0, aligned, down):
    """(backing uint8 [H, pitch, 4] filled with 0x5A, its [:, :W] canvas view, step_rows, step_cols)"""
    step_rows, step_cols = (h + 1, 0) if down else (0, w + 2)
    height = row0 + (n - 1) * step_rows + h + 3
    width = col0 + (n - 1) * step_cols + w + 5
    pitch = (width + 3) // 4 * 4 + (0 if aligned else 1)
    backing = torch.full((height, pitch, 4), FILL, dtype=torch.uint8, device=DEV)
    assert backing.data_ptr() % 16 == 0 and (backing.stride(0) % 16 == 0) == aligned
    return backing, backing[:, :width], step_rows, step_cols


def _expected(backing_shape, panels, n, h, w, row0, col0, step_rows, step_cols):
    exp = np.full(backing_shape, FILL, dtype=np.uint8)
    for i in range(n):
        r, c = row0 + i * step_rows, col0 + i * step_cols
        exp[r:r + h, c:c + w] = panels[i]
    return exp


def _rgb_pool():
    k = np.arange(256, dtype=np.float64)
    unit = (k / 255).astype(np.float32)                         # the bin edges of the unit mode
    return np.concatenate([RO.edge_values_rgb(), unit, np.nextafter(unit, np.float32(-9)),
                           np.nextafter(unit, np.float32(9)), np.array([np.inf, -np.inf, np.nan], dtype=np.float32)])


@pytest.mark.parametrize("kind", SOURCES)
@pytest.mark.parametrize("n,h,w", GEOMETRIES)
def test_render_rgb_every_byte(n, h, w, kind):
    from floodgan import ops
    rng = np.random.default_rng(n * 1000 + h * 100 + w)
    src, host = _source(kind, _values(_rgb_pool(), n * 9 * h * (w + 5), rng), n, h, w)
    ref = {mode: RO.rgb_bytes(host[:, :3].transpose(0, 2, 3, 1), mode) for mode in ("signed", "unit")}
    for j, (row0, col0, aligned, down) in enumerate(PLACEMENTS):
        mode = "unit" if j % 4 == 3 else "signed"
        backing, canvas, sr, sc = _canvas(n, h, w, row0, col0, aligned, down)
        ops.render_rgb(src, canvas, row0, col0, unit=mode == "unit", step_rows=sr, step_cols=sc)
        got = backing.cpu().numpy()
        exp = _expected(got.shape, ref[mode], n, h, w, row0, col0, sr, sc)
        assert np.array_equal(got, exp), (mode, row0, col0, aligned, down, np.argwhere(got != exp)[:4].tolist())


def _scalar_source(kind, values, n, h, w):
    dev, host = _source(kind, values, n, h, w)
    return dev, host[:, 0]


@pytest.mark.parametrize("kind", SOURCES)
@pytest.mark.parametrize("n,h,w", GEOMETRIES)
def test_render_scalar_every_byte(n, h, w, kind):
    from floodgan import ops
    from floodgan.render import device_lut
    rng = np.random.default_rng(n * 1000 + h * 100 + w + 7)
    size = n * 9 * h * (w + 5)
    pool = np.concatenate([RO.edge_values_scalar(), np.array([np.inf, -np.inf, np.nan], dtype=np.float32)])
    unit_src, unit_host = _scalar_source(kind, _values(pool, size, rng), n, h, w)
    logits = (rng.standard_normal(size) * 2).astype(np.float32)
    logits[np.abs(logits) <= RO.LOGIT_BAND] = 1.0               # the band has a test of its own
    logit_src, logit_host = _scalar_source(kind, logits, n, h, w)
    cases = [("unit", "gray_r", unit_src, unit_host), ("unit", "gray", unit_src, unit_host),
             ("threshold", "gray", unit_src, unit_host), ("logit", "gray", logit_src, logit_host)]
    for j, (row0, col0, aligned, down) in enumerate(PLACEMENTS):
        skind, cmap, src, host = cases[j % 4]
        backing, canvas, sr, sc = _canvas(n, h, w, row0, col0, aligned, down)
        ops.render_scalar(src, device_lut(cmap, DEV), canvas, row0, col0, kind=skind, step_rows=sr, step_cols=sc)
        got = backing.cpu().numpy()
        exp = _expected(got.shape, RO.scalar_bytes(host, cmap, skind), n, h, w, row0, col0, sr, sc)
        assert np.array_equal(got, exp), (skind, cmap, row0, col0, aligned, down, np.argwhere(got != exp)[:4].tolist())
    # every (kind, colormap) also at every alignment class of the column
    for skind, cmap, src, host in cases:
        for col0 in (0, 1, 3, 4):
            backing, canvas, sr, sc = _canvas(n, h, w, 2, col0, True, True)
            ops.render_scalar(src, device_lut(cmap, DEV), canvas, 2, col0, kind=skind, step_rows=sr, step_cols=sc)
            got = backing.cpu().numpy()
            exp = _expected(got.shape, RO.scalar_bytes(host, cmap, skind), n, h, w, 2, col0, sr, sc)
            assert np.array_equal(got, exp), (skind, cmap, col0)


def _band_logits(n, h, w, seed):
    """random logits with exactly 8 values inside |x| <= 2^-21 and values just outside it"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n * h * w) * 2).astype(np.float32)
    x[np.abs(x) <= 4 * RO.LOGIT_BAND] = 0.25
    b = np.float32(RO.LOGIT_BAND)
    inside = np.array([0.0, -0.0, b, -b, b / 2, -b / 2, 1e-42, 3e-8], dtype=np.float32)
    outside = np.array([np.nextafter(b, np.float32(1)), -np.nextafter(b, np.float32(1)), 2 * b, -2 * b, 1e-6, -1e-6],
                       dtype=np.float32)
    pos = rng.permutation(x.size)[:len(inside) + len(outside)]
    x[pos] = np.concatenate([inside, outside])
    assert int((np.abs(x) <= RO.LOGIT_BAND).sum()) == 8 and x.size >= 4096
    return x.reshape(n, h, w)


def test_render_logit_mask_band_and_confusion_count():
    """outside |x| <= 2^-21 the rendered mask is torch.sigmoid(x) > 0.5 on the CPU; inside, either table entry; and the
    white pixels are exactly fg_mask_confusion's predicted positives (tp + fp): one device function decides both"""
    from floodgan.evaluate import MaskConfusion
    from floodgan.plans import Buf
    from floodgan.render import Canvas
    n, h, w = 2, 40, 67
    x = _band_logits(n, h, w, 5)
    pred = Buf.zeros(n, h, w, 4, 0, DEV)
    pred.interior()[..., 0] = torch.from_numpy(x).to(DEV)
    truth = Buf.zeros(n, h, w, 4, 0, DEV)
    truth.interior()[..., 0] = torch.from_numpy(np.random.default_rng(6).standard_normal((n, h, w))
                                                .astype(np.float32)).to(DEV)
    cv = Canvas(n * h, w, DEV).scalar(pred, 0, 0, cmap="gray", kind="logit", step_rows=h)
    got = cv.host().copy().reshape(n, h, w, 4)
    table = RO.lut("gray")
    white, black = (got == table[255]).all(-1), (got == table[0]).all(-1)
    assert (white | black).all()
    band = np.abs(x) <= RO.LOGIT_BAND
    ref = (torch.sigmoid(torch.from_numpy(x)) > 0.5).numpy()
    assert np.array_equal(white[~band], ref[~band])
    mc = MaskConfusion(DEV)
    mc.update(pred, truth)
    tp, fp, tn, fn = (int(v) for v in mc.counts.cpu())
    assert tp + fp == int(white.sum()) and tn + fn == int(black.sum())
    # the strided-tensor route (channel 0 of an NCHW view) renders the same picture
    cv2 = Canvas(n * h, w, DEV).scalar(torch.from_numpy(x).to(DEV), 0, 0, cmap="gray", kind="logit", step_rows=h)
    assert np.array_equal(cv2.host().reshape(n, h, w, 4), got)


def _raw_rgb(src, n, h, w, canvas_ptr, height, width, row_bytes, row0, col0, sr=0, sc=0):
    from floodgan import _lib as L
    from floodgan import ops
    return L.load().fg_render_rgb(ops.sview(src), n, h, w, L.FG_RENDER_SIGNED,
                                  L.fg_canvas(canvas_ptr, height, width, row_bytes), row0, col0, sr, sc,
                                  L.stream_handle())


def _raw_scalar(src, n, h, w, canvas_ptr, height, width, row_bytes, row0, col0, sr=0, sc=0):
    from floodgan import _lib as L
    from floodgan import ops
    from floodgan.render import device_lut
    return L.load().fg_render_scalar(ops.sview(src), n, h, w, L.FG_SCALAR_UNIT, L.ptr(device_lut("gray", DEV)),
                                     L.fg_canvas(canvas_ptr, height, width, row_bytes), row0, col0, sr, sc,
                                     L.stream_handle())


@pytest.mark.parametrize("raw", [_raw_rgb, _raw_scalar])
def test_invalid_calls_fail_and_leave_the_canvas_untouched(raw):
    from floodgan import _lib as L
    n, h, w = 2, 6, 8
    src = torch.rand(n, 3, h, w, device=DEV)
    H, W = 20, 24
    backing = torch.full((H, W, 4), FILL, dtype=torch.uint8, device=DEV)
    p, rb = backing.data_ptr(), 4 * W
    bad = [dict(row0=0, col0=W - w + 1),                      # over the right edge
           dict(row0=H - h + 1, col0=0),                      # over the bottom edge
           dict(row0=-1, col0=0), dict(row0=0, col0=-1),      # over the top / left edge
           dict(row0=0, col0=0, sr=H - h + 1),                  # the second panel of the batch leaves the canvas
           dict(row0=H - h, col0=0, sr=-(H - h) - 1),         # ... through a negative step
           dict(row0=0, col0=0, sc=W - w + 1),
           dict(row0=0, col0=0, row_bytes=4 * W - 4),         # rows shorter than the canvas is wide
           dict(row0=0, col0=0, n=0), dict(row0=0, col0=0, h=0), dict(row0=0, col0=0, w=-3),
           dict(row0=0, col0=0, height=0), dict(row0=0, col0=0, width=0)]
    for kw in bad:
        a = dict(n=n, h=h, w=w, height=H, width=W, row_bytes=rb, sr=0, sc=0)
        a.update(kw)
        rc = raw(src, a["n"], a["h"], a["w"], p, a["height"], a["width"], a["row_bytes"], a["row0"], a["col0"],
                 a["sr"], a["sc"])
        assert rc == -1, kw
        assert L.load().fg_last_error().decode().startswith("fg_render_"), kw
    torch.cuda.synchronize()
    assert bool((backing == FILL).all())
    # the same geometry placed inside succeeds
    assert raw(src, n, h, w, p, H, W, rb, H - 2 * h, W - w, h, 0) == 0
    got = backing.cpu().numpy()
    assert (got[H - 2 * h:, W - w:] != FILL).any() and (got[:H - 2 * h] == FILL).all() and (got[:, :W - w] == FILL).all()
    # and the Python layer raises the library's message
    from floodgan import ops
    with pytest.raises(RuntimeError, match="leaves the"):
        ops.render_rgb(src, backing, H - h + 1, 0)


# ------------------------------------------------------------------------------------------ the reference's methods

def _dataset(root, names, size, seed=11):
    """tiles in the reference's layout (dataset_input/<image>_10m.tif, 9 channels; dataset_output/<image>.tif) and a
    split table with one row per image"""
    from floodgan.data import write_tile
    rng = np.random.default_rng(seed)
    for d in ("dataset_input", "dataset_output", "metadata"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    rows = ["image,best_DEM,same_DEM,version,split,disaster,country"]
    for name in names:
        write_tile(os.path.join(root, "dataset_input", f"{name}_10m.tif"), rng.random((size, size, 9)).astype(np.float32))
        write_tile(os.path.join(root, "dataset_output", f"{name}.tif"), rng.random((size, size, 3)).astype(np.float32))
        rows.append(f"{name},10m,10m,original,train,hurricane-harvey,usa")
    csv = os.path.join(root, "metadata", "dataset_split.csv")
    with open(csv, "w") as f:
        f.write("\n".join(rows) + "\n")
    return csv


def _png(path):
    from floodgan.png import read_png
    return read_png(path)


def _signed(t):
    """oracle bytes of an [1, C, H, W] device tensor's first three channels"""
    return RO.rgb_bytes(t[0, :3].permute(1, 2, 0).cpu().numpy(), "signed")


NAMES = ["hurricane-harvey_00000000", "hurricane-harvey_00000001"]


def test_model_plot_image(tmp_path):
    from floodgan.data import load_image_pair
    from floodgan.model import Model
    from floodgan.render import PANELS_KEY, sheet_layout
    root = str(tmp_path)
    csv = _dataset(root, NAMES, 64)
    m = Model(model="PairedAttention", training_model=False, data_path=root, resize=None, crop=None, csv_path=csv,
              train_loader=[], device=DEV)
    name = NAMES[1]
    x, y, shown = load_image_pair(name, root, "best", "all", None, None, 0, csv_path=csv, device=DEV)
    assert shown == name and tuple(x.shape) == (1, 9, 64, 64) and tuple(y.shape) == (1, 3, 64, 64)
    torch.manual_seed(47)
    with torch.no_grad():
        out = m.generator(x)
    mask = m.generator.last_attention_mask
    want = {"input": _signed(x), "ground truth": _signed(y), "output": _signed(out),
            "attention mask": RO.scalar_bytes(mask[0].cpu().numpy(), "gray_r", "unit")}
    singles = {}
    for kind in want:
        written = m.plot_image(name, kind, False)
        assert list(written) == [kind]
        singles[kind], text = _png(written[kind])
        assert text == {} and np.array_equal(singles[kind], want[kind]), kind
    base = os.path.join(root, "images")
    assert written["attention mask"].startswith(f"{base}/PairedAttention_{name}_attentionMask_epoch0_allTopography_")
    assert os.path.exists(f"{base}/{name}_input.png") and os.path.exists(f"{base}/{name}_groundTruth.png")
    assert len([f for f in os.listdir(base) if f.startswith(f"PairedAttention_{name}_epoch0_")]) == 1
    with pytest.raises(NotImplementedError, match="Type of image"):
        m.plot_image(name, "heat map", False)
    # the image set: one row, four columns, the single images at the layout's offsets, white gutters
    written = m.plot_image(name, None, True)
    sheet, text = _png(written["set"])
    height, width, off = sheet_layout(1, 4, 64, 64)
    assert sheet.shape == (height, width, 4) == (64, 4 * 64 + 3 * 8, 4)
    covered = np.zeros((height, width), dtype=bool)
    for c, kind in enumerate(["input", "output", "attention mask", "ground truth"]):
        r0, c0 = off[0][c]
        assert np.array_equal(sheet[r0:r0 + 64, c0:c0 + 64], singles[kind]), kind
        covered[r0:r0 + 64, c0:c0 + 64] = True
    assert (sheet[~covered] == 255).all() and int((~covered).sum()) == 3 * 8 * 64
    panels = json.loads(text[PANELS_KEY])
    assert panels["columns"] == ["Input", "Generator Output", "Attention Mask", "Ground Truth Output"]
    assert panels["rows"] == [name] and panels == m.last_panels
    # a model without attention has no attention mask to plot (the reference's error)
    torch.manual_seed(1)
    c = Model(model="CycleGAN", training_model=False, data_path=root, resize=None, crop=None, csv_path=csv,
              train_loader=[], device=DEV)
    with pytest.raises(NotImplementedError, match="Type of image"):
        c.plot_image(name, "attention mask", False)
    sheet3, text3 = _png(c.plot_image(name, None, True)["set"])
    assert sheet3.shape == (64, 3 * 64 + 2 * 8, 4)
    assert json.loads(text3[PANELS_KEY])["columns"] == ["Input", "Generator Output", "Ground Truth Output"]


def _batches(n_batches, batch, size, seed):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand((batch, 9, size, size), generator=g) * 2 - 1).to(DEV),
             (torch.rand((batch, 3, size, size), generator=g) * 2 - 1).to(DEV),
             [f"hurricane-harvey_{seed}{i}{k}" for k in range(batch)]) for i in range(n_batches)]


def test_model_plot_sample_images(tmp_path):
    from floodgan.model import Model
    from floodgan.render import PANELS_KEY
    train, val = _batches(3, 1, 32, 1), _batches(3, 1, 32, 2)
    m = Model(model="PairedAttention", training_model=False, data_path=str(tmp_path), resize=32, train_loader=train,
              val_loader=val, device=DEV)
    paths = m.plot_sample_images(2, use_test_data=False)
    state = torch.get_rng_state()
    torch.manual_seed(47)
    assert torch.equal(state, torch.get_rng_state())              # PairedAttention draws nothing after the last seed
    assert len(paths) == 2 and "_training_epoch0_" in paths[0] and "_validation_epoch0_" in paths[1]
    for path, loader in zip(paths, (train, val)):
        sheet, text = _png(path)
        assert sheet.shape == (2 * 32 + 8, 4 * 32 + 3 * 8, 4)
        panels = json.loads(text[PANELS_KEY])
        assert panels["rows"] == [loader[0][2][0], loader[1][2][0]] and len(panels["columns"]) == 4
        for r in range(2):
            x, y, _ = loader[r]
            torch.manual_seed(47)
            with torch.no_grad():
                out = m.generator(x)
            r0 = r * 40
            assert np.array_equal(sheet[r0:r0 + 32, 0:32], _signed(x))
            assert np.array_equal(sheet[r0:r0 + 32, 40:72], _signed(out))
            assert np.array_equal(sheet[r0:r0 + 32, 80:112],
                                  RO.scalar_bytes(m.generator.last_attention_mask[0].cpu().numpy(), "gray_r", "unit"))
            assert np.array_equal(sheet[r0:r0 + 32, 120:152], _signed(y))
        assert (sheet[32:40] == 255).all()
    with pytest.raises(RuntimeError, match="test loader"):
        m.plot_sample_images(2, use_test_data=True)


def test_save_images_interval_does_not_disturb_training(tmp_path):
    from floodgan.model import Model
    params = []
    for interval in (1, 0):
        root = str(tmp_path / f"run{interval}")
        os.makedirs(root)
        train, val = _batches(2, 2, 32, 3), _batches(2, 2, 32, 4)
        m = Model(model="PairedAttention", num_epochs=1, data_path=root, resize=32, train_loader=train, val_loader=val,
                  save_images_interval=interval, device=DEV)
        m.train_paired()
        torch.cuda.synchronize()
        images = os.path.join(root, "images")
        if interval:
            files = sorted(os.listdir(images))
            assert len(files) == 2 and "_training_epoch1_" in files[0] and "_validation_epoch1_" in files[1], files
            assert _png(os.path.join(images, files[0]))[0].shape == (2 * 32 + 8, 4 * 32 + 3 * 8, 4)
        else:
            assert not os.path.exists(images) or not os.listdir(images)
        params.append([p.detach().cpu().clone() for net in (m.generator, m.discriminator) for p in net.parameters()])
    assert len(params[0]) == len(params[1]) and all(torch.equal(a, b) for a, b in zip(*params))


def _seg_model(root, **kw):
    from floodgan.segmentation import SegmentationModel
    torch.manual_seed(5)
    m = SegmentationModel(data_path=root, device=DEV, verbose=False, **kw)
    m.model.eval()
    return m


def test_segmentation_plot_mask_image(tmp_path):
    from floodgan.png import write_png
    root = str(tmp_path)
    rgb = np.random.default_rng(8).integers(0, 256, (64, 64, 4), dtype=np.uint8)
    src = os.path.join(root, "scene.png")
    write_png(src, rgb)
    m = _seg_model(root)
    path = m.plot_mask_image(src)
    assert os.path.basename(path).startswith("SegmentationMask_scene_") and os.path.dirname(path) == f"{root}/images"
    got, _ = _png(path)
    table = RO.lut("gray")
    white, black = (got == table[255]).all(-1), (got == table[0]).all(-1)
    assert got.shape == (64, 64, 4) and (white | black).all()
    x = torch.from_numpy((rgb[:, :, :3].astype(np.float32) / np.float32(255)).transpose(2, 0, 1).copy())[None].to(DEV)
    with torch.no_grad():
        logits = m.model(x)[0, 0].cpu()
    band = (logits.abs() <= RO.LOGIT_BAND).numpy()
    assert band.mean() < 0.01
    ref = (torch.sigmoid(logits) > 0.5).numpy()
    assert np.array_equal(white[~band], ref[~band])


def test_segmentation_plot_sample_images(tmp_path):
    from floodgan.render import PANELS_KEY, save_image
    from floodgan.segmentation import unit_image_passthrough
    root = str(tmp_path)
    g = torch.Generator().manual_seed(12)
    items = [(torch.rand((1, 3, 64, 64), generator=g) * 1.4 - 0.2, torch.rand((1, 1, 64, 64), generator=g), [f"{k}.tif"])
             for k in "ab"]
    m = _seg_model(root, save_images_interval=1)                  # no longer raises
    assert m.save_images_interval == 1
    m.val_loader = items
    path = m.plot_sample_images(2)
    sheet, text = _png(path)
    assert sheet.shape == (2 * 64 + 8, 3 * 64 + 2 * 8, 4)
    panels = json.loads(text[PANELS_KEY])
    assert panels["columns"] == ["Input", "Ground Truth Mask", "Predicted Mask"] and panels["rows"] == ["a.tif", "b.tif"]
    for r, (x, t, _) in enumerate(items):
        x, t = x.to(DEV), t.to(DEV)
        logits = m.model.logits_from_buf(unit_image_passthrough(x)[1])
        singles = [_png(save_image(os.path.join(root, f"s{k}.png"), src, kind, **kw))[0]
                   for k, (src, kind, kw) in enumerate([(x, "rgb", dict(unit=True)), (t, "mask_true", {}),
                                                        (logits, "mask_logits", {})])]
        assert np.array_equal(singles[0], RO.rgb_bytes(x[0].permute(1, 2, 0).cpu().numpy(), "unit"))
        assert np.array_equal(singles[1], RO.scalar_bytes(t[0, 0].cpu().numpy(), "gray", "threshold"))
        for c in range(3):
            assert np.array_equal(sheet[r * 72:r * 72 + 64, c * 72:c * 72 + 64], singles[c]), (r, c)
    assert (sheet[64:72] == 255).all() and (sheet[:, 64:72] == 255).all()


def test_compare_output_images(tmp_path):
    import floodgan
    from floodgan.data import load_image_pair
    from floodgan.model import Model
    from floodgan.render import PANELS_KEY
    root = str(tmp_path)
    csv = _dataset(root, NAMES, 128, seed=13)
    torch.manual_seed(3)
    gens = {"PairedAttention": floodgan.PairedAttentionGenerator(input_channels=9).apply(Model.initialise_weights).to(DEV),
            "CycleGAN": floodgan.CycleGANGenerator(input_channels=9).apply(Model.initialise_weights).to(DEV)}
    out_path = os.path.join(root, "compare.png")
    panels = floodgan.compare_output_images(gens, [NAMES[0] + "_0", NAMES[1]], compare="model", data_path=root,
                                            dataset_dem="best", topography="all", resize=None, crop=4, crop_index=3,
                                            csv_path=csv, out_path=out_path, device=DEV)
    sheet, text = _png(out_path)
    assert sheet.shape == (2 * 64 + 8, 4 * 64 + 3 * 8, 4)
    assert json.loads(text[PANELS_KEY]) == panels
    assert panels["columns"] == ["Input", "Ground truth", "PairedAttention", "CycleGAN"]
    assert panels["rows"] == [NAMES[0] + "_0", NAMES[1] + "_3"]
    for r, (name, ci) in enumerate([(NAMES[0], 0), (NAMES[1], 3)]):
        x, y, _ = load_image_pair(name, root, "best", "all", None, 4, ci, csv_path=csv, device=DEV)
        assert tuple(x.shape) == (1, 9, 64, 64)
        assert np.array_equal(sheet[r * 72:r * 72 + 64, 0:64], _signed(x))
        assert np.array_equal(sheet[r * 72:r * 72 + 64, 72:136], _signed(y))
        for c, gen in enumerate(gens.values(), start=2):
            torch.manual_seed(47)
            with torch.no_grad():
                out = gen(x)
            assert np.array_equal(sheet[r * 72:r * 72 + 64, c * 72:c * 72 + 64], _signed(out)), (r, c)
