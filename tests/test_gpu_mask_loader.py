"""The staged segmentation loader on the GPU (floodgan.data.MaskTileLoader over fg_mask_tile_batch).  The kernel is a
pure copy (np.fliplr of the flipped tiles, HWC -> CHW), so every comparison here is bit-exact (torch.equal): the
kernel against numpy, the loader's batches against the default DataLoader's, and a SegmentationModel trained through
the staged loader against one trained through the default loader."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch

from tiff_util import write_tiff

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0          # tile values lie in [0, 1)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ------------------------------------------------------------------------------------------ kernel

SHAPES = [(1, 1, 1), (2, 3, 4), (3, 2, 5), (2, 5, 7), (4, 4, 8), (2, 16, 16), (3, 17, 33), (64, 2, 3)]
FLIPS = {"none": lambda n: [False] * n, "all": lambda n: [True] * n, "alternating": lambda n: [k % 2 == 1 for k in range(n)]}


def _dest(kind, n, c, h, w):
    """an [n, c, h, w] view inside a sentinel-filled buffer: (buffer, view, floats before the view).  The buffer's
    own base is 16-byte aligned (asserted); `offset` moves the view one float off that alignment"""
    pad = 9 if kind == "offset" else 8
    buf = torch.full((pad + n * c * h * w + 8,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0
    body = buf[pad:pad + n * c * h * w]
    view = body.view(n, c, h, w) if kind == "nchw" else body.view(n, h, w, c).permute(0, 3, 1, 2)
    return buf, view, pad


def _reference(img, msk, flips):
    """np.fliplr / transpose of MaskDataset.__getitem__ (floodgan/data.py), per tile"""
    xs = [np.fliplr(a) if f else a for a, f in zip(img, flips)]
    ms = [np.fliplr(a) if f else a for a, f in zip(msk, flips)]
    return (torch.from_numpy(np.stack([a.transpose(2, 0, 1).copy() for a in xs])),
            torch.from_numpy(np.stack([a.copy() for a in ms]))[:, None])


@pytest.mark.parametrize("kind", ["channels_last", "nchw", "offset"])
@pytest.mark.parametrize("flip", list(FLIPS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_batch_bit_exact(shape, flip, kind):
    from floodgan import _lib as L
    from floodgan.data import mask_batch
    n, h, w = shape
    rng = np.random.default_rng(n * 1000 + h * 100 + w)
    img = rng.random((n, h, w, 3), dtype=np.float32)
    msk = rng.random((n, h, w), dtype=np.float32)
    flips = FLIPS[flip](n)
    ibuf, iview, ipad = _dest(kind, n, 3, h, w)
    mbuf, mview, mpad = _dest(kind, n, 1, h, w)
    mask_batch(torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV), flips, iview, mview)
    launched = L.last_launch()
    torch.cuda.synchronize()
    # the wide kernel takes exactly the unit-stride channels-last, 16-byte aligned, width % 4 == 0 case
    assert launched == ("mask_tile_runs" if kind == "channels_last" and w % 4 == 0 else "mask_tile_pixels")
    want_i, want_m = _reference(img, msk, flips)
    assert torch.equal(iview.cpu(), want_i)
    assert torch.equal(mview.cpu(), want_m)
    for buf, pad, numel in ((ibuf, ipad, n * 3 * h * w), (mbuf, mpad, n * h * w)):
        host = buf.cpu()
        assert bool((host[:pad] == SENTINEL).all()) and bool((host[pad + numel:] == SENTINEL).all())


def test_mask_batch_splits_more_than_64_tiles():
    from floodgan.data import mask_batch
    n, h, w = 67, 2, 4
    rng = np.random.default_rng(67)
    img, msk = rng.random((n, h, w, 3), dtype=np.float32), rng.random((n, h, w), dtype=np.float32)
    flips = [k % 3 == 0 for k in range(n)]
    out_i = torch.empty((n, 3, h, w), device=DEV, memory_format=torch.channels_last)
    out_m = torch.empty((n, 1, h, w), device=DEV)
    mask_batch(torch.from_numpy(img).to(DEV), torch.from_numpy(msk).to(DEV), flips, out_i, out_m)
    want_i, want_m = _reference(img, msk, flips)
    assert torch.equal(out_i.cpu(), want_i) and torch.equal(out_m.cpu(), want_m)


@pytest.mark.parametrize("case", ["n65", "zero_h", "zero_w", "short_image_stride", "short_mask_stride"])
def test_mask_tile_batch_rejects_before_launching(case):
    """n over the flip mask's 64 bits, a zero size and a tile stride shorter than a tile are refused by the host-side
    checks: the call returns the error and launches nothing (the outputs keep their sentinel)"""
    from floodgan import _lib as L
    n, h, w = (65, 2, 4) if case == "n65" else (2, 2, 4)
    img = torch.zeros(65 * 2 * 4 * 3, device=DEV)
    msk = torch.zeros(65 * 2 * 4, device=DEV)
    out_i = torch.full((65, 3, 2, 4), SENTINEL, device=DEV)
    out_m = torch.full((65, 1, 2, 4), SENTINEL, device=DEV)
    istride, mstride = h * w * 3, h * w
    if case == "zero_h":
        h = 0
    if case == "zero_w":
        w = 0
    if case == "short_image_stride":
        istride -= 1
    if case == "short_mask_stride":
        mstride -= 1
    rc = L.load().fg_mask_tile_batch(img.data_ptr(), istride, msk.data_ptr(), mstride, n, h, w, 0,
                                     L.fg_wview(out_i.data_ptr(), *out_i.stride()),
                                     L.fg_wview(out_m.data_ptr(), *out_m.stride()), L.stream_handle())
    assert rc != 0
    with pytest.raises(RuntimeError, match="fg_mask_tile_batch"):
        L.check(rc, "mask_tile_batch")
    torch.cuda.synchronize()
    assert bool((out_i == SENTINEL).all()) and bool((out_m == SENTINEL).all())
    assert L.load().fg_mask_tile_batch(None, istride, msk.data_ptr(), mstride, 1, 2, 4, 0,
                                       L.fg_wview(out_i.data_ptr(), *out_i.stride()),
                                       L.fg_wview(out_m.data_ptr(), *out_m.stride()), L.stream_handle()) != 0


# ------------------------------------------------------------------------------------------ loader

def _tree(root, sizes, rows, seed=12, channels=None):
    """tiles {name: (h, w)} under root/masks_input, root/masks_output and the metadata table `rows` of
    (image, split, version); channels: {name: image channels} where not 3"""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "masks_input"))
    os.makedirs(os.path.join(root, "masks_output"))
    for name, (h, w) in sizes.items():
        c = (channels or {}).get(name, 3)
        write_tiff(os.path.join(root, "masks_input", name), rng.random((h, w, c), dtype=np.float32))
        write_tiff(os.path.join(root, "masks_output", name), (rng.random((h, w)) > 0.5).astype(np.float32))
    csv = os.path.join(root, "masks_metadata.csv")
    with open(csv, "w") as f:
        f.write("image,split,version,country\n" + "".join(f"{i},{s},{v},usa\n" for i, s, v in rows))
    return csv


def _five_tiles(root):
    names = [f"t{i}.tif" for i in range(5)]
    rows = [(n, "train", "original") for n in names] + [(n, "train", "flipped") for n in names[:3]]
    return _tree(root, {n: (16, 24) for n in names}, rows)


def _in_thread(fn, timeout=60):
    """run fn in a worker thread joined with a timeout: a stuck producer fails the test instead of stalling it"""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:
            box["error"] = e
    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(timeout)
    assert not th.is_alive(), "the loader did not finish"
    if "error" in box:
        raise box["error"]
    return box["value"]


def test_staged_batches_equal_the_dataloaders(tmp_path):
    from floodgan.data import MaskTileLoader, create_masks_dataset
    root = str(tmp_path)
    csv = _five_tiles(root)
    stock, _, _ = create_masks_dataset("usa", root, True, batch_size=2, csv_path=csv)
    staged, _, _ = create_masks_dataset("usa", root, True, batch_size=2, csv_path=csv, staged=True, device=DEV,
                                        prefetch=1)
    assert type(staged) is MaskTileLoader and len(staged) == len(stock) == 4
    torch.manual_seed(3)
    want = [(x.clone(), t.clone(), list(names)) for _ in range(2) for x, t, names in stock]

    def run():
        torch.manual_seed(3)
        got, held = [], []
        for _ in range(2):
            for x, t, names in staged:
                assert x.is_cuda and t.is_cuda and x.dtype == t.dtype == torch.float32
                assert x.is_contiguous(memory_format=torch.channels_last) and t.is_contiguous()
                for s in staged._slots:                      # fresh tensors: no alias of the ring
                    for d in (s.dx, s.dy):
                        lo, hi = d.data_ptr(), d.data_ptr() + d.numel() * 4
                        assert not (lo <= x.data_ptr() < hi) and not (lo <= t.data_ptr() < hi)
                got.append((x.cpu(), t.cpu(), list(names)))
                held.append((x, t))
        return got, held
    got, held = _in_thread(run)
    assert len(staged._slots) == 2 and len(got) == 8 > len(staged._slots)          # the slots were reused
    assert [g[2] for g in got] == [w[2] for w in want]
    for (gx, gt, _), (wx, wt, _) in zip(got, want):
        assert gx.shape == wx.shape and torch.equal(gx, wx) and torch.equal(gt, wt)
    torch.cuda.synchronize()
    for (x, t), (wx, wt, _) in zip(held, want):              # still the same after every later batch was drawn
        assert torch.equal(x.cpu(), wx) and torch.equal(t.cpu(), wt)


def test_early_exit_then_a_full_epoch(tmp_path):
    from floodgan.data import create_masks_dataset
    root = str(tmp_path)
    csv = _five_tiles(root)
    staged, _, _ = create_masks_dataset("usa", root, True, batch_size=1, csv_path=csv, staged=True, device=DEV,
                                        prefetch=1)

    def run():
        first = None
        for _, _, names in staged:
            first = names
            break
        threads = threading.active_count()
        with pytest.raises(KeyError):
            for _ in staged:
                raise KeyError("loop body")
        return first, sorted(n for _, _, names in staged for n in names), threads, threading.active_count()
    first, epoch, t0, t1 = _in_thread(run)
    assert len(first) == 1
    assert epoch == sorted([f"t{i}.tif" for i in range(5)] + [f"t{i}.tif" for i in range(3)])
    assert t1 <= t0                                          # no producer left behind


def test_producer_error_reaches_the_consumer(tmp_path):
    from floodgan.data import MaskDataset, MaskTileLoader
    root = str(tmp_path)
    _five_tiles(root)
    ds = MaskDataset([("t0.tif", "original"), ("t1.tif", "flipped"), ("absent.tif", "original"),
                      ("t2.tif", "original")], root)
    loader = MaskTileLoader(ds, batch_size=1, shuffle=False, device=DEV, prefetch=1)

    def run():
        seen = []
        with pytest.raises(RuntimeError, match="cannot open file"):
            for _, _, names in loader:
                seen += names
        return seen
    assert _in_thread(run) == ["t0.tif", "t1.tif"]


@pytest.mark.parametrize("odd", ["size", "channels", "first_channels"])
def test_geometry_errors_name_the_tile(tmp_path, odd):
    from floodgan.data import MaskDataset, MaskTileLoader
    root = str(tmp_path)
    sizes = {"a.tif": (16, 24), "b.tif": (16, 24), "odd.tif": (16, 32) if odd == "size" else (16, 24)}
    _tree(root, sizes, [], channels=None if odd == "size" else {"odd.tif": 4})
    order = ["odd.tif", "a.tif", "b.tif"] if odd == "first_channels" else ["a.tif", "odd.tif", "b.tif"]
    loader = MaskTileLoader(MaskDataset([(n, "original") for n in order], root), batch_size=1, shuffle=False,
                            device=DEV, prefetch=1)

    def run():
        with pytest.raises((RuntimeError, ValueError), match="odd.tif"):
            for _ in loader:
                pass
        return True
    assert _in_thread(run)


# ------------------------------------------------------------------------------------------ model

def _model_run(root, csv, staged):
    from floodgan.segmentation import SegmentationModel
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(31)
        m = SegmentationModel(data_path=root, train=True, num_epochs=2, device=DEV, verbose=False, csv_path=csv,
                              staged_loader=staged)
        m.train_model()
    return m


def _pictures(m):
    df = m.calculate_metrics()
    with open(m.plot_sample_images(2), "rb") as f:
        return df, f.read()


def _gap(a, b):
    """the largest absolute difference between two runs' (losses, accuracies, state_dict)"""
    la = max(abs(x - y) for x, y in zip(a.all_losses + a.all_accuracies, b.all_losses + b.all_accuracies))
    sa, sb = a.model.state_dict(), b.model.state_dict()
    return max(la, max(float((sa[k].double() - sb[k].double()).abs().max()) for k in sa))


def test_model_trains_the_same_through_either_loader(tmp_path, report):
    """SegmentationModel(staged_loader=True) against the default model from the same seed, two epochs over three
    32x32 training items.  The default model is run twice first: where those runs are bit-identical the staged run
    must be bit-identical to them; otherwise it is bounded by the difference the two default runs show."""
    from floodgan.data import MaskTileLoader
    roots, csvs = [], []
    for k in range(3):                                       # one identical tree per model (each writes under its own)
        roots.append(str(tmp_path / f"run{k}"))
        os.makedirs(roots[-1])
        rows = [("a.tif", "train", "original"), ("a.tif", "train", "flipped"), ("b.tif", "train", "original"),
                ("c.tif", "validation", "original"), ("d.tif", "test", "flipped")]
        csvs.append(_tree(roots[-1], {f"{n}.tif": (32, 32) for n in "abcd"}, rows, seed=21))
    d0, d1 = _model_run(roots[0], csvs[0], False), _model_run(roots[1], csvs[1], False)
    st = _model_run(roots[2], csvs[2], True)
    assert type(st.train_loader) is MaskTileLoader and type(st.val_loader) is MaskTileLoader
    assert len(st.all_losses) == len(d0.all_losses) == 2 and np.isfinite(st.all_losses).all()
    spread = _gap(d0, d1)
    report("seg_staged_loader_vs_default", default_run_to_run=spread, staged_vs_default=_gap(st, d0))
    if spread == 0.0:
        assert st.all_losses == d0.all_losses and st.all_accuracies == d0.all_accuracies
        for (k, a), (_, b) in zip(st.model.state_dict().items(), d0.model.state_dict().items()):
            assert torch.equal(a, b), k
    else:
        assert _gap(st, d0) <= spread
        st.model.load_state_dict(d0.model.state_dict())      # the pictures below: from equal weights
    df_d, png_d = _pictures(d0)
    df_s, png_s = _pictures(st)
    assert df_d.equals(df_s) and list(df_d.columns) == list(df_s.columns)
    assert png_d == png_s
