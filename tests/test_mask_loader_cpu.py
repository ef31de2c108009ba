"""The staged segmentation loader's host side (floodgan.data.MaskTileLoader), without a device: MaskDataset.item, the
batch order against a real DataLoader(MaskDataset, shuffle=True), and the unchanged defaults of create_masks_dataset
and SegmentationModel.  Constructing a MaskTileLoader allocates nothing (its ring is made by the first iteration)."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from tiff_util import write_tiff


def _tiles(root, names, h=2, w=4):
    rng = np.random.default_rng(8)
    os.makedirs(root / "masks_input")
    os.makedirs(root / "masks_output")
    for name in names:
        write_tiff(str(root / "masks_input" / name), rng.random((h, w, 3), dtype=np.float32))
        write_tiff(str(root / "masks_output" / name), (rng.random((h, w)) > 0.5).astype(np.float32))


def test_mask_dataset_item(tmp_path):
    from floodgan.data import MaskDataset
    ds = MaskDataset([("a.tif", "original"), ("a.tif", "flipped"), ("b.tif", "flipped")], str(tmp_path))
    for i, (name, flipped) in enumerate((("a.tif", False), ("a.tif", True), ("b.tif", True))):
        assert ds.item(i) == (f"{tmp_path}/masks_input/{name}", f"{tmp_path}/masks_output/{name}", flipped, name)


@pytest.mark.parametrize("batch_size", [1, 2, 3])
def test_order_is_the_dataloaders(tmp_path, batch_size):
    from floodgan.data import MaskDataset, MaskTileLoader
    names = [f"{i}.tif" for i in range(7)]
    _tiles(tmp_path, names)
    ds = MaskDataset([(n, "original") for n in names], str(tmp_path))
    staged = MaskTileLoader(ds, batch_size=batch_size, shuffle=True)
    assert staged._slots is None and staged.dataset is ds and staged.batch_size == batch_size
    stock = DataLoader(ds, batch_size=batch_size, shuffle=True)
    assert len(staged) == len(stock) == -(-7 // batch_size)
    for seed in (0, 1, 47, 2024):
        torch.manual_seed(seed)
        want = [[names.index(n) for n in batch_names] for _, _, batch_names in stock]
        torch.manual_seed(seed)
        got = list(staged._batches())
        assert got == want, (seed, got, want)
        assert len(got[-1]) == 7 - batch_size * (len(got) - 1)            # the short last batch is kept
    assert staged._slots is None


def _mask_tree(root):
    _tiles(root, [f"{n}.tif" for n in "abc"], 16, 16)
    rows = [("a.tif", "train", "original", "usa"), ("a.tif", "train", "flipped", "usa"),
            ("b.tif", "validation", "original", "usa"), ("c.tif", "test", "original", "usa")]
    csv = root / "masks_metadata.csv"
    csv.write_text("image,split,version,country\n" + "".join(",".join(r) + "\n" for r in rows))
    return str(csv)


def test_defaults_are_dataloaders(tmp_path):
    from floodgan.data import MaskTileLoader, create_masks_dataset
    from floodgan.segmentation import SegmentationModel
    csv = _mask_tree(tmp_path)
    for loader in create_masks_dataset("usa", str(tmp_path), False, csv_path=csv, staged=False):
        assert type(loader) is DataLoader
    m = SegmentationModel(data_path=str(tmp_path), train=True, device="cpu", num_epochs=1, verbose=False, csv_path=csv)
    assert m.staged_loader is False
    assert all(type(ld) is DataLoader for ld in (m.train_loader, m.val_loader, m.test_loader))
    train, val, test = create_masks_dataset("usa", str(tmp_path), False, batch_size=2, csv_path=csv, staged=True)
    assert all(type(ld) is MaskTileLoader and ld._slots is None for ld in (train, val, test))
    assert (len(train.dataset), len(val.dataset), len(test.dataset), train.batch_size, len(train)) == (2, 1, 1, 2, 1)
    train, val, test = create_masks_dataset("usa", str(tmp_path), True, csv_path=csv, staged=True)
    assert type(train) is MaskTileLoader and val is None and test is None and len(train) == 4
