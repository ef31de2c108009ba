"""The segmentation model's training LOOP on one MI355X: SegmentationModel.train_model() fed by the default loader
(arm "default": DataLoader(MaskDataset), host decode / flip / transpose / collate / pin / blocking copy on the training
thread) and by the staged loader (arm "staged": MaskTileLoader, staged_loader=True), beside the step alone on
tensors that already sit on the device (arm "step": what scripts/bench_seg_train.py times; arm "step_read" adds the
loop's per-batch read of loss and accuracy, a device-to-host copy that waits for the step).  DESIGN.md §8 holds the
table.

The data is 8 seeded synthetic 1024x1024 tile pairs (fp32 TIFF, floodgan.data.write_tile), each listed as `original`
and `flipped` (16 items), written to a temporary directory and read back from the page cache: this measures the
loader, not storage.  All arms run in one process, warmed up, alternating by round; one round is one epoch
(train_model() with one epoch left to run) and is timed with a host clock around work that ends in a device
synchronise.  Needs a HIP device: there is no CPU measurement path.
  python scripts/bench_seg_loader.py [--rounds 5] [--tiles 8] [--res 1024]
  python scripts/bench_seg_loader.py --arms staged --rounds 2     (one arm alone: the form a kernel profiler wraps)"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flood-prediction-gan_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ARMS = ["default", "staged", "step", "step_read"]


def write_tree(root, tiles, res):
    from floodgan.data import write_tile
    rng = np.random.default_rng(77)
    os.makedirs(os.path.join(root, "masks_input"))
    os.makedirs(os.path.join(root, "masks_output"))
    rows = ["image,split,version,country"]
    for i in range(tiles):
        name = f"tile_{i:04d}.tif"
        write_tile(os.path.join(root, "masks_input", name), rng.random((res, res, 3), dtype=np.float32))
        write_tile(os.path.join(root, "masks_output", name), (rng.random((res, res)) > 0.6).astype(np.float32))
        rows += [f"{name},train,original,usa", f"{name},train,flipped,usa"]
    csv = os.path.join(root, "masks_metadata.csv")
    with open(csv, "w") as f:
        f.write("\n".join(rows) + "\n")
    return csv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds (epochs) per arm")
    ap.add_argument("--warmup", type=int, default=1, help="untimed rounds per arm")
    ap.add_argument("--tiles", type=int, default=8, help="tile pairs; each is listed original and flipped")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--arms", default=",".join(ARMS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_loader needs a HIP device: there is no CPU measurement path")
    from floodgan.segmentation import SegmentationModel, SegStep
    names = a.arms.split(",")
    assert names and all(n in ARMS for n in names), names
    items = 2 * a.tiles
    with tempfile.TemporaryDirectory() as root:
        csv = write_tree(root, a.tiles, a.res)

        def model(**kw):
            torch.manual_seed(5)
            m = SegmentationModel(train=True, device="cuda", verbose=False, num_epochs=1000, csv_path=csv, **kw)
            m.model.train()
            return m

        def loop(m):                                     # one epoch of the loop a user runs
            def run():
                m.starting_epoch = m.num_epochs                 # the last epoch: the learning rate stays put
                m.train_model()
            return run

        def resident(read):
            m = model()
            g = torch.Generator().manual_seed(77)
            x = torch.rand((1, 3, a.res, a.res), generator=g).cuda()
            t = (torch.rand((1, 1, a.res, a.res), generator=g) > 0.6).float().cuda()

            def run():
                for _ in range(items):
                    res = m.step_fn(x, t)
                    if read:
                        SegStep.read(res, t.numel())
            return run

        make = {"default": lambda: loop(model(data_path=root, train_on_all=True)),
                "staged": lambda: loop(model(data_path=root, train_on_all=True, staged_loader=True)),
                "step": lambda: resident(False), "step_read": lambda: resident(True)}
        arms = {n: make[n]() for n in names}
        ms = {n: [] for n in names}
        for r in range(a.warmup + a.rounds):
            for n, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    ms[n].append(1e3 * (time.perf_counter() - t0) / items)
    px = a.res * a.res
    out = {"what": "segmentation training loop, ms per item (batch 1), host clock around one epoch ending in a "
                   "synchronise; arms alternate by round; tiles read from the page cache",
           "res": a.res, "items_per_round": items, "rounds": a.rounds, "torch": torch.__version__,
           # fg_mask_tile_batch reads and writes every float of the image and mask tile once
           "mask_tile_batch_bytes_per_item": 2 * 4 * (3 * px + px), "h2d_bytes_per_item": 4 * (3 * px + px)}
    for n, v in ms.items():
        out[n] = {"ms_per_item_median": round(statistics.median(v), 3), "ms_per_item_min": round(min(v), 3),
                  "ms_per_item_max": round(max(v), 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
