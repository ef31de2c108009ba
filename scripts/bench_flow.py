"""Time of the flow-routing stage (floodgan.flow) on scenes of 1024^2 and 2048^2.

Inputs   terraces   floor(8 x) of a low-pass noise field x in [0, 1]: wide flats, the realistic hard case; timed with
                    flat_rounds 0 and 64
         noise      independent uniform pixels: a pit every few pixels, paths of a few steps, so nearly every pointer
                    of the doubling is -1 after the first rounds
         spiral     a one-pixel trench that descends one unit per step along a rectangular spiral between higher walls:
                    one path of about H W / 2 steps, alive in every doubling round, no confluence
         cone       the squared distance to the centre: one pit that the whole scene drains to (the largest confluence)
Arms     directions    ops.flow_directions into a plane allocated before (one launch)
         flats         ops.flow_flats, 64 rounds (the copy of the plane, the clearing of the counts and 64 launches);
                       terraces only
         accumulate    ops.flow_accumulate into planes allocated before (the scratch allocation, 1 + 2 K launches and
                       copies)
         whole         floodgan.flow_accumulation of the elevation: the three above, the allocations and the device ->
                       host reads of the counts
Device events around each sample, a warm-up of every arm first, REPEATS samples, the median reported, and its share of
the scene times DESIGN.md §17 records (16.4 ms at 1024^2, 42.8 ms at 2048^2).  Nothing here is a gate.
    python scripts/bench_flow.py
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flood-prediction-gan_amd"))

from floodgan import flow_accumulation, ops  # noqa: E402

SCENE_MS = {1024: 16.4, 2048: 42.8}
WARMUP, REPEATS = 3, 15
FLAT_ROUNDS = 64


def smooth(R, dev, seed):
    g = torch.Generator().manual_seed(seed)
    field = torch.randn((1, 1, R, R), generator=g).to(dev)
    for _ in range(3):                                   # three box blurs of 31 pixels: a smooth field
        field = torch.nn.functional.avg_pool2d(field, 31, stride=1, padding=15)
    return field[0, 0]


def spiral(R):
    """the trench's coordinates in path order: runs of R - 1, R - 1, R - 1, R - 3, R - 3, R - 5, ... steps, turning
    right, so that one wall pixel stays between two turns"""
    ys, xs = [np.zeros(1, dtype=np.int64)], [np.zeros(1, dtype=np.int64)]
    y = x = 0
    runs = [R - 1] + [n for k in range(R - 1, 0, -2) for n in (k, k)][:-1]
    for turn, n in enumerate(runs):
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[turn % 4]
        steps = np.arange(1, n + 1)
        ys.append(y + dy * steps)
        xs.append(x + dx * steps)
        y, x = y + dy * n, x + dx * n
    ys, xs = np.concatenate(ys), np.concatenate(xs)
    z = np.full((R, R), float(len(ys) + 7), dtype=np.float32)
    z[ys, xs] = np.arange(len(ys) - 1, -1, -1, dtype=np.float32)
    return z


def inputs(R, dev):
    g = torch.Generator().manual_seed(R)
    field = smooth(R, dev, R)
    unit = (field - field.min()) / (field.max() - field.min())
    y, x = torch.meshgrid(torch.arange(R, device=dev), torch.arange(R, device=dev), indexing="ij")
    return {"terraces": torch.floor(8 * unit).contiguous(),
            "noise": torch.rand((R, R), generator=g).to(dev),
            "spiral": torch.from_numpy(spiral(R)).to(dev),
            "cone": ((y - R // 2) ** 2 + (x - R // 2) ** 2).float().contiguous()}


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


def main():
    dev = "cuda"
    results = []
    for R, scene_ms in SCENE_MS.items():
        d0, d1 = (torch.empty((R, R), dtype=torch.uint8, device=dev) for _ in range(2))
        acc, basin, length = (torch.empty((R, R), dtype=torch.int32, device=dev) for _ in range(3))
        counts = torch.empty(FLAT_ROUNDS, dtype=torch.int32, device=dev)
        for name, elev in inputs(R, dev).items():
            for flat_rounds in ((0, FLAT_ROUNDS) if name == "terraces" else (0,)):
                res = flow_accumulation(elev, flat_rounds=flat_rounds)
                row = {"size": R, "input": name, "flat_rounds": flat_rounds, "rounds": res["rounds"],
                       "pit_count": res["pit_count"], "max_length": int(res["length"].max()),
                       "max_accumulation": int(res["accumulation"].max()),
                       "flat_directed": int(res["flat_directed"].sum())}
                directions = res["directions"]
                arms = {"directions": lambda: ops.flow_directions(elev, d0),
                        "accumulate": lambda: ops.flow_accumulate(directions, acc, basin, length),
                        "whole": lambda: flow_accumulation(elev, flat_rounds=flat_rounds)}
                if flat_rounds:
                    ops.flow_directions(elev, d0)
                    arms["flats"] = lambda: ops.flow_flats(elev, d0, FLAT_ROUNDS, d1, counts)
                for arm, fn in arms.items():
                    ms = median_ms(fn)
                    row[arm] = {"median_ms": ms, "share_of_scene": round(ms / scene_ms, 4)}
                results.append(row)
                print(json.dumps(row), flush=True)
    print(json.dumps({"warmup": WARMUP, "repeats": REPEATS, "scene_ms": SCENE_MS, "results": results}))


if __name__ == "__main__":
    main()
