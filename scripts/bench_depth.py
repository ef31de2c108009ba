"""Time of the flood-depth stage (floodgan.depth) on scenes of 1024^2 and 2048^2.

Inputs   blob       a thresholded low-pass noise field (the field of scripts/bench_regions.py): the realistic case
         corner     one seed in the top-left corner: every pixel's nearest seed is a whole scene away
         bernoulli  independent pixels, p = 0.5: the nearest seed is a step or two away
         top_row    the first row all seeds: the longest search of the row pass (every column holds a candidate, so
                    a pixel of row y has to look y columns to each side before it may stop)
Arms     nearest_seed  floodgan.nearest_seed of the input as the seed plane (three launches and the scratch allocation)
         depth         floodgan.flood_depth with the input as the flood mask and a smooth elevation: shore, transform
                       of the shore plane, depth, the scene's totals and their device -> host reads
         depth+table   the same with the regions of the mask (their table launches are not part of the sample)
         scipy         scipy.ndimage.distance_transform_edt(return_indices=True) of the host seed plane plus the
                       device -> host copy of the plane, for orientation (wall clock)
Device events around each sample, a warm-up of every arm first, REPEATS samples, the median reported, and its share of
the scene times DESIGN.md §17 records (16.4 ms at 1024^2, 42.8 ms at 2048^2).  Nothing here is a gate.
    python scripts/bench_depth.py
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flood-prediction-gan_amd"))

from floodgan import flood_depth, flood_regions, nearest_seed  # noqa: E402

SCENE_MS = {1024: 16.4, 2048: 42.8}
WARMUP, REPEATS = 3, 15


def smooth(R, dev, seed):
    g = torch.Generator().manual_seed(seed)
    field = torch.randn((1, 1, R, R), generator=g).to(dev)
    for _ in range(3):                                   # three box blurs of 31 pixels: a smooth field
        field = torch.nn.functional.avg_pool2d(field, 31, stride=1, padding=15)
    return (field / field.std()).contiguous()


def inputs(R, dev):
    g = torch.Generator().manual_seed(R)
    blob = (smooth(R, dev, R) > 0).float()
    corner = torch.zeros((1, 1, R, R), device=dev)
    corner[0, 0, 0, 0] = 1.0
    bern = (torch.rand((1, 1, R, R), generator=g).to(dev) < 0.5).float()
    top = torch.zeros((1, 1, R, R), device=dev)
    top[0, 0, 0] = 1.0
    return {"blob": blob, "corner": corner, "bernoulli": bern, "top_row": top}


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


def scipy_arm(plane):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    times = []
    for _ in range(3):
        t = time.perf_counter()
        host = plane[0, 0].cpu().numpy()
        ndimage.distance_transform_edt(host <= 0.5, return_indices=True)
        times.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(times), 3)}


def main():
    dev = "cuda"
    results = []
    for R, scene_ms in SCENE_MS.items():
        elevation = (smooth(R, dev, R + 1)[0, 0] * 4 + 20).contiguous()
        for name, plane in inputs(R, dev).items():
            regions = flood_regions(plane, "threshold", 1, 0, 8)
            arms = {"nearest_seed": lambda: nearest_seed(plane, "threshold", True),
                    "depth": lambda: flood_depth(plane, elevation),
                    "depth+table": lambda: flood_depth(plane, elevation, regions)}
            res = arms["depth"]()
            row = {"size": R, "input": name, "seeds": int(plane.sum()), "shore_count": res["shore_count"],
                   "regions": regions["count"], "max_depth": round(res["max_depth"], 4)}
            for arm, fn in arms.items():
                ms = median_ms(fn)
                row[arm] = {"median_ms": ms, "share_of_scene": round(ms / scene_ms, 4)}
            row["scipy_edt_plus_copy"] = scipy_arm(plane)
            results.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({"warmup": WARMUP, "repeats": REPEATS, "scene_ms": SCENE_MS, "results": results}))


if __name__ == "__main__":
    main()
