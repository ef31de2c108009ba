"""Time of the flood-region stage (floodgan.regions) on scenes of 1024^2 and 2048^2 logits.

Inputs   blob       a thresholded low-pass noise field: the realistic case (few, large, smooth regions)
         bernoulli  independent pixels, p = 0.593: the adversarial case (near the site-percolation threshold)
         flood      every pixel flood: one region, the most contended statistics
Arms     sieve+table   flood_regions(min_region=16, min_hole=16, connectivity=8)
         sieve         the same with table=False
         plain+table   flood_regions(min_region=1, min_hole=0): one labelling and the table, no sieve
         stages        the entries alone, device time without the host's reads: label (3 launches), stats, apply,
                       table (rank plane made beforehand)
         scipy         scipy.ndimage.label of the host mask plus the device -> host copy of the logits, for orientation
                       (wall clock; it labels once and does neither the sieve nor the table)
Device events around each sample of the device arms (the sample includes the stage's own device -> host reads), a
warm-up of every arm first, REPEATS samples, the median reported, and its share of the scene times DESIGN.md §17
records (16.4 ms at 1024^2, 42.8 ms at 2048^2).  Nothing here is a gate.
    python scripts/bench_regions.py
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flood-prediction-gan_amd"))

from floodgan import flood_regions, ops  # noqa: E402
from floodgan.regions import region_table  # noqa: E402

SCENE_MS = {1024: 16.4, 2048: 42.8}
WARMUP, REPEATS = 3, 15
MIN_REGION = MIN_HOLE = 16


def inputs(R, dev):
    g = torch.Generator().manual_seed(R)
    noise = torch.randn((1, 1, R, R), generator=g).to(dev)
    blob = noise
    for _ in range(3):                                   # three box blurs of 31 pixels: a smooth field
        blob = torch.nn.functional.avg_pool2d(blob, 31, stride=1, padding=15)
    blob = (blob / blob.std() * 4).contiguous()
    bern = torch.where(torch.rand((1, 1, R, R), generator=g).to(dev) < 0.593, 4.0, -4.0)
    return {"blob": blob, "bernoulli": bern, "flood": torch.full((1, 1, R, R), 4.0, device=dev)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    return round(statistics.median(timed(fn) for _ in range(REPEATS)), 4)


def stages(z):
    """device time of each entry alone on z (no sieve: the flood class of z itself)"""
    _, _, H, W = z.shape
    dev = z.device
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    area, border = torch.empty_like(labels), torch.empty_like(labels)
    mask = torch.empty((1, 1, H, W), device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    out = {"label": median_ms(lambda: ops.regions_label(z, "logit", True, 8, labels)),
           "label_dry": median_ms(lambda: ops.regions_label(z, "logit", False, 8, labels))}
    ops.regions_label(z, "logit", True, 8, labels)
    out["stats"] = median_ms(lambda: ops.regions_stats(labels, area, border))
    out["apply"] = median_ms(lambda: ops.regions_apply(labels, area, border, "remove", MIN_REGION, mask, counts))
    roots = torch.nonzero(labels.view(-1) == torch.arange(H * W, dtype=torch.int32, device=dev)).view(-1)
    rank = torch.empty_like(labels)
    rank.view(-1)[roots] = torch.arange(roots.numel(), dtype=torch.int32, device=dev)
    table = torch.empty((roots.numel(), 8), dtype=torch.int64, device=dev)
    out["table"] = median_ms(lambda: ops.regions_table(labels, rank, table))
    out["rank_plumbing"] = median_ms(lambda: region_table(labels)) - out["table"]
    return out


def scipy_arm(z):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    times = []
    for _ in range(3):
        t = time.perf_counter()
        host = z[0, 0].cpu().numpy()
        _, n = ndimage.label(host > 0, structure=[[1, 1, 1]] * 3)
        times.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(times), 3), "components": int(n)}


def main():
    dev = "cuda"
    results = []
    for R, scene_ms in SCENE_MS.items():
        for name, z in inputs(R, dev).items():
            arms = {"sieve+table": lambda: flood_regions(z, "logit", MIN_REGION, MIN_HOLE, 8),
                    "sieve": lambda: flood_regions(z, "logit", MIN_REGION, MIN_HOLE, 8, table=False),
                    "plain+table": lambda: flood_regions(z, "logit", 1, 0, 8)}
            res = arms["sieve+table"]()
            row = {"size": R, "input": name, "regions": res["count"], "removed": res["removed"],
                   "filled": res["filled"], "flood_fraction": round(res["flood_fraction"], 4)}
            for arm, fn in arms.items():
                ms = median_ms(fn)
                row[arm] = {"median_ms": ms, "share_of_scene": round(ms / scene_ms, 4)}
            row["stages_ms"] = stages(z)
            row["scipy_label_plus_copy"] = scipy_arm(z)
            results.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({"min_region": MIN_REGION, "min_hole": MIN_HOLE, "connectivity": 8, "warmup": WARMUP,
                      "repeats": REPEATS, "scene_ms": SCENE_MS, "results": results}))


if __name__ == "__main__":
    main()
