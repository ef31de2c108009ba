"""The host side of segmentation-model training (floodgan.segmentation.SegmentationModel(train=True),
floodgan.data's mask data path) and the planner geometry its backward adds (ConvTranspose2d(2, 2) backward, the
channel-sliced input gradient of a decoder level's cat), on the CPU."""
import gzip
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from floodgan import plans as PL
from floodgan.plans import Buf
from test_plans_cpu import close, emu_conv, emu_pack, emu_reduce, emu_wgrad, from_buf, to_buf
from tiff_util import write_tiff

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gold():
    z = np.load(os.path.join(GOLDEN_DIR, "segtrain_32.npz"), allow_pickle=False)
    return {k.replace("__", "."): z[k] for k in z.files}


def _model(**kw):
    from floodgan.segmentation import SegmentationModel
    return SegmentationModel(train=True, device="cpu", verbose=False, **kw)


@pytest.mark.parametrize("num_epochs", [1, 4, 100])
def test_lambda_rule_matches_reference(num_epochs):
    m = _model(num_epochs=num_epochs)
    ref = _gold()[f"lambda_rule_{num_epochs}"]
    mine = np.array([m.lambda_rule(e) for e in range(num_epochs + 1)])
    formula = np.array([1.0 - max(0, e + 1 - (num_epochs / 2)) / float((num_epochs / 2) + 1)
                        for e in range(num_epochs + 1)])
    assert np.array_equal(mine, ref) and np.array_equal(mine, formula)


def test_train_true_constructs():
    from floodgan.optim import FusedAdam
    m = _model(num_epochs=4)
    assert isinstance(m.optimizer, FusedAdam)
    g = m.optimizer.param_groups[0]
    assert g["lr"] == 1e-4 and tuple(g["betas"]) == (0.5, 0.999)
    assert m.starting_epoch == 1 and m.train is True
    lrs = []
    for _ in range(4):
        lrs.append(m.optimizer.param_groups[0]["lr"])
        m.scheduler.step()
    assert np.allclose(lrs, [1e-4 * m.lambda_rule(e) for e in range(4)], rtol=1e-12)


def test_train_model_without_data_raises():
    with pytest.raises(RuntimeError, match="no training data"):
        _model().train_model()


def test_checkpoint_keys_and_round_trip(tmp_path):
    m = _model(num_epochs=6, data_path=None, save_model_interval=1)
    m.data_path = str(tmp_path)
    with torch.no_grad():
        m.model.inc.double_conv[1].running_mean.add_(0.25)
    path = m.save_results(3, [0.5, 0.7], [0.25, 0.75], 0.0)
    assert os.path.basename(path).startswith("SegmentationModel_epoch3_usaData_date") and path.endswith(".pth.tar")
    assert os.path.dirname(path) == str(tmp_path / "models")
    saved = torch.load(path, weights_only=True)
    assert set(saved) == {"current_epoch", "num_epochs", "model", "all_losses", "all_accuracies"}
    assert saved["current_epoch"] == 4 and saved["num_epochs"] == 6
    assert saved["all_losses"] == [pytest.approx(0.6)] and saved["all_accuracies"] == [0.5]
    m2 = _model(pretrained_model_path=path)
    assert (m2.current_epoch, m2.starting_epoch, m2.num_epochs) == (4, 4, 6)
    assert m2.all_losses == saved["all_losses"] and m2.all_accuracies == saved["all_accuracies"]
    for (k, a), (_, b) in zip(m.model.state_dict().items(), m2.model.state_dict().items()):
        assert torch.equal(a, b), k
    # the evaluation side reads the same file
    from floodgan.segmentation import SegmentationModel
    m3 = SegmentationModel(pretrained_model_path=path, device="cpu")
    assert torch.equal(m3.model.inc.double_conv[1].running_mean, m.model.inc.double_conv[1].running_mean)
    # no checkpoint off the interval
    m.save_model_interval = 2
    assert m.save_results(5, [1.0], [1.0], 0.0) is None


@pytest.mark.parametrize("subset", ["usa", "india"])
@pytest.mark.parametrize("train_on_all", [False, True])
def test_determine_masks_dataset(subset, train_on_all):
    from floodgan.data import determine_masks_dataset
    with gzip.open(os.path.join(GOLDEN_DIR, "masks_splits.json.gz"), "rt") as f:
        ref = json.load(f)[f"{subset}/{int(train_on_all)}"]
    got = determine_masks_dataset(subset, train_on_all, csv_path=os.path.join(GOLDEN_DIR, "masks_metadata.csv"))
    assert len(got) == 3
    for mine, theirs in zip(got, ref):
        if theirs is None:
            assert mine is None
        else:
            assert [list(t) for t in mine] == theirs
    assert got[0]
    with pytest.raises(NotImplementedError):
        determine_masks_dataset("all", False, csv_path=os.path.join(GOLDEN_DIR, "masks_metadata.csv"))


def test_mask_dataset(tmp_path):
    from floodgan.data import MaskDataset
    rng = np.random.default_rng(3)
    os.makedirs(tmp_path / "masks_input")
    os.makedirs(tmp_path / "masks_output")
    tiles = {}
    for name, (h, w) in (("a.tif", (16, 24)), ("b.tif", (8, 8))):
        img = rng.random((h, w, 3), dtype=np.float32)
        mask = (rng.random((h, w)) > 0.5).astype(np.float32)
        write_tiff(str(tmp_path / "masks_input" / name), img)
        write_tiff(str(tmp_path / "masks_output" / name), mask)
        tiles[name] = (img, mask)
    ds = MaskDataset([("a.tif", "original"), ("a.tif", "flipped"), ("b.tif", "flipped")], str(tmp_path))
    assert len(ds) == 3
    for i, (name, flipped) in enumerate((("a.tif", False), ("a.tif", True), ("b.tif", True))):
        x, t, got_name = ds[i]
        img, mask = tiles[name]
        if flipped:
            img, mask = np.fliplr(img), np.fliplr(mask)
        assert got_name == name and x.dtype == torch.float32 and t.dtype == torch.float32
        assert x.shape == (3,) + mask.shape and t.shape == (1,) + mask.shape
        assert np.array_equal(x.numpy(), img.transpose(2, 0, 1)) and np.array_equal(t.numpy()[0], mask)
        assert x.is_contiguous() and t.is_contiguous()


# ------------------------------------------------------------------------------ planner geometry (emulated engine)

torch.manual_seed(0)


@pytest.mark.parametrize("cin,H,W", [(8, 5, 3), (16, 2, 2)])
def test_convT2_backward_plans(cin, H, W):
    """ConvTranspose2d(k=2, s=2, p=0): input gradient as one k=2 stride-2 conv of the (unpadded) gradient, weight
    gradient by wgrad_convT with p=0"""
    cout = cin // 2
    x = torch.randn(2, cin, H, W, requires_grad=True)
    w = torch.randn(cin, cout, 2, 2, requires_grad=True)
    y = F.conv_transpose2d(x, w, stride=2)
    gy = torch.randn_like(y)
    gx_ref, gw_ref = torch.autograd.grad(y, (x, w), gy)
    G = to_buf(gy, 0, "constant")
    m = PL.wmap_convT_dgrad(w.shape, G.c)
    Y = Buf(torch.zeros(2 * H * W * cin), 2, H, W, cin, 0)
    emu_conv(PL.conv_problem(G, 0, 2, 2, emu_pack(w.detach(), m), m, Y))
    assert close(from_buf(Y), gx_ref)
    X = to_buf(x.detach(), 1, "constant")                       # the forward's input keeps its zero border
    slab = emu_wgrad(PL.wgrad_convT(X, G, 2, 0, cin))
    dw = torch.zeros_like(w)
    emu_reduce(slab, PL.wmap_wgrad(w.shape, True, G.c, 2), dw)
    assert close(dw, gw_ref)


def test_conv_dgrad_channel_halves():
    """the 3x3 input gradient of a conv over torch.cat([skip, up], 1), one problem per half"""
    c = 4
    x = torch.randn(2, 2 * c, 6, 5, requires_grad=True)
    w = torch.randn(6, 2 * c, 3, 3)
    y = F.conv2d(x, w, padding=1)
    gy = torch.randn_like(y)
    (ref,) = torch.autograd.grad(y, x, gy)
    G = to_buf(gy, 1, "constant", c_alloc=8)
    for c0 in (0, c):
        m = PL.wmap_conv_dgrad_s1_part(w.shape, G.c, c0, c)
        Y = Buf(torch.zeros(2 * 6 * 5 * c), 2, 6, 5, c, 0)
        emu_conv(PL.conv_problem(G, 1, 3, 1, emu_pack(w, m), m, Y))
        assert close(from_buf(Y), ref[:, c0:c0 + c])


# ------------------------------------------------------------------------------ the script's constructor call

def _segment_py_kwargs(**over):
    """exactly the keywords the reference's segment.py passes: SegmentationModel(**vars(args)) of its parser"""
    kw = dict(train=True, dataset_subset="usa", train_on_all=False, data_path=None, num_epochs=1,
              save_model_interval=0, save_images_interval=0, verbose=False, pretrained_model_path=None,
              plot_mask_image=None, seed=47, use_test_data=False)
    kw.update(over)
    return kw


def test_constructs_with_the_scripts_keywords():
    from floodgan import segmentation as segmentation_model       # the documented switch of segment.py's import
    import inspect
    params = inspect.signature(segmentation_model.SegmentationModel.__init__).parameters
    assert params["device"].default == "cuda"                     # the script passes no device
    m = segmentation_model.SegmentationModel(device="cpu", **_segment_py_kwargs())
    assert m.train is True and m.num_epochs == 1 and m.use_test_data is False and m.seed == 47
    assert m.train_loader is None                                 # data_path None: loaders are assigned
    m = segmentation_model.SegmentationModel(device="cpu", **_segment_py_kwargs(train=False, use_test_data=True))
    assert m.train is False and m.use_test_data is True and not hasattr(m, "optimizer")


@pytest.mark.parametrize("over", [dict(save_images_interval=5), dict(plot_mask_image="tile.png")])
def test_plot_keywords_raise_out_of_scope(over):
    from floodgan.segmentation import SegmentationModel
    with pytest.raises(NotImplementedError, match="out of scope"):
        SegmentationModel(device="cpu", **_segment_py_kwargs(**over))


def _mask_tree(root):
    """a tiny masks dataset: tiles under masks_input / masks_output and its metadata table"""
    rng = np.random.default_rng(4)
    os.makedirs(root / "masks_input")
    os.makedirs(root / "masks_output")
    rows = [("a.tif", "train", "original", "usa"), ("a.tif", "train", "flipped", "usa"),
            ("b.tif", "validation", "original", "usa"), ("c.tif", "test", "original", "usa"),
            ("d.tif", "train", "original", "india"), ("b.tif", "validation", "flipped", "india"),
            ("c.tif", "test", "flipped", "india")]
    for name in "abcd":
        write_tiff(str(root / "masks_input" / f"{name}.tif"), rng.random((16, 16, 3), dtype=np.float32))
        write_tiff(str(root / "masks_output" / f"{name}.tif"), (rng.random((16, 16)) > 0.5).astype(np.float32))
    csv = root / "masks_metadata.csv"
    csv.write_text("image,split,version,country\n" + "".join(",".join(r) + "\n" for r in rows))
    return str(csv)


def test_create_masks_dataset(tmp_path):
    from floodgan.data import create_masks_dataset
    csv = _mask_tree(tmp_path)
    train, val, test = create_masks_dataset("usa", str(tmp_path), False, csv_path=csv)
    assert (len(train.dataset), len(val.dataset), len(test.dataset)) == (2, 1, 1)
    assert train.batch_size == 1                                   # the reference's default
    seen = sorted((names[0], tuple(x.shape), tuple(t.shape)) for x, t, names in train)
    assert seen == [("a.tif", (1, 3, 16, 16), (1, 1, 16, 16))] * 2
    assert [names[0] for _, _, names in val] == ["b.tif"] and [names[0] for _, _, names in test] == ["c.tif"]
    train, val, test = create_masks_dataset("usa", str(tmp_path), True, batch_size=2, csv_path=csv)
    assert val is None and test is None and len(train.dataset) == 4
    assert sorted(x.shape[0] for x, _, _ in train) == [2, 2]


def test_train_true_with_data_path_builds_loaders(tmp_path):
    csv = _mask_tree(tmp_path)
    m = _model(data_path=str(tmp_path), dataset_subset="india", csv_path=csv)
    assert len(m.train_loader.dataset) == 1 and len(m.val_loader.dataset) == 1 and len(m.test_loader.dataset) == 1
    (x, t, names), = list(m.train_loader)
    assert names[0] == "d.tif" and x.shape == (1, 3, 16, 16) and t.shape == (1, 1, 16, 16)
    m = _model(data_path=str(tmp_path), train_on_all=True, csv_path=csv)
    assert len(m.train_loader.dataset) == 4 and m.val_loader is None and m.test_loader is None
