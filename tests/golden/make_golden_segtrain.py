"""Golden vectors for training the flood-segmentation UNet from the REAL reference class.

Runs only in the build container (see make_golden.py): imports the reference's own models/segmentation_model.py
(third-party modules the step never touches are replaced by make_golden's inert stand-ins), builds
SegmentationModel(train=True, num_epochs=4) under torch.manual_seed(5), replaces its train_loader with synthetic
batches and drives the UNMODIFIED train_model() (models/segmentation_model.py:250-277) for 2 epochs of 2 batches,
(1, 3, 32, 32) then (2, 3, 32, 48); the loader ends the run when a third epoch asks for data.  save_results is
wrapped (on the instance) to read what train_model hands it.

Only numbers are written (tests/golden/segtrain_32.npz): per-batch loss and accuracy, the learning rate in effect in
each epoch, the reference's lambda_rule for num_epochs in {1, 4, 100}, and per-tensor parameter / buffer checksums at
initialisation and after each epoch.  Also recorded here, as data for the CPU tests: determine_masks_dataset's lists
(tests/golden/masks_splits.json.gz) from the reference's metadata/masks_metadata.csv, copied beside it.

Usage:  python tests/golden/make_golden_segtrain.py
"""
import gzip
import json
import os
import shutil
import sys

import numpy as np
import torch

from make_golden import HERE, REF, _install_stubs, checksums

EPOCHS, NUM_EPOCHS = 2, 4


def synth_batches():
    g = torch.Generator().manual_seed(77)
    out = []
    for shape in ((1, 3, 32, 32), (2, 3, 32, 48)):
        x = torch.rand(shape, generator=g)
        t = (torch.rand((shape[0], 1) + shape[2:], generator=g) > 0.6).float()
        out.append((x, t, ["synthetic"] * shape[0]))
    return out


class _Done(Exception):
    pass


class _Loader:
    def __init__(self, batches, epochs):
        self.batches, self.left = batches, epochs

    def __iter__(self):
        if self.left == 0:
            raise _Done
        self.left -= 1
        return iter(self.batches)


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    _install_stubs()
    os.chdir(REF)                                   # the reference reads metadata/*.csv relative to the cwd
    from models import data as D  # noqa: E402  (reference, imported read-only)
    from models import segmentation_model as SM  # noqa: E402
    torch.set_num_threads(8)
    rec = {}
    torch.manual_seed(5)
    m = SM.SegmentationModel(num_epochs=NUM_EPOCHS, train=True, verbose=False, data_path=None)
    for k, v in checksums(m.model).items():
        rec["init/" + k] = v
    m.train_loader = _Loader(synth_batches(), EPOCHS)
    ep_losses, ep_accs, lrs = [], [], [m.optimizer.param_groups[0]["lr"]]
    orig = m.save_results

    def record(epoch, losses, accuracies, epoch_start_time):
        ep_losses.append(list(losses))
        ep_accs.append(list(accuracies))
        lrs.append(m.optimizer.param_groups[0]["lr"])          # after scheduler.step(): the next epoch's
        for k, v in checksums(m.model).items():
            rec[f"epoch{epoch}/" + k] = v
        orig(epoch=epoch, losses=losses, accuracies=accuracies, epoch_start_time=epoch_start_time)

    m.save_results = record
    try:
        m.train_model()
    except _Done:
        pass
    assert len(ep_losses) == EPOCHS
    rec["losses"] = np.array(ep_losses, np.float64)             # [epoch, batch]
    rec["accuracies"] = np.array(ep_accs, np.float64)
    rec["lr"] = np.array(lrs[:EPOCHS], np.float64)              # in effect during each epoch
    rec["all_losses"] = np.array(m.all_losses, np.float64)
    rec["all_accuracies"] = np.array(m.all_accuracies, np.float64)
    for n in (1, 4, 100):
        m.num_epochs = n
        rec[f"lambda_rule_{n}"] = np.array([m.lambda_rule(e) for e in range(n + 1)], np.float64)
    out = os.path.join(HERE, "segtrain_32.npz")
    np.savez_compressed(out, **{k.replace(".", "__"): v for k, v in rec.items()})
    print("wrote", out, os.path.getsize(out), "bytes")

    splits = {}
    for subset in ("usa", "india"):
        for all_ in (False, True):
            tr, va, te = D.determine_masks_dataset(subset, all_)
            splits[f"{subset}/{int(all_)}"] = [None if s is None else [list(t) for t in s] for s in (tr, va, te)]
    with gzip.open(os.path.join(HERE, "masks_splits.json.gz"), "wt") as f:
        json.dump(splits, f)
    shutil.copyfile(os.path.join(REF, "metadata", "masks_metadata.csv"), os.path.join(HERE, "masks_metadata.csv"))
    print("wrote masks_splits.json.gz, masks_metadata.csv")


if __name__ == "__main__":
    main()
