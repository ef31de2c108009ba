"""Time of the outline stage (floodgan.outline) on the labels of scenes of 1024^2 and 2048^2.

Inputs   blob, bernoulli, flood   those of scripts/bench_regions.py: the realistic smooth field, independent pixels
                                  at p = 0.593 and the all-flood scene
         spiral                   a one-pixel-wide rectangular spiral: one ring of about H W edges, the longest a scene
                                  allows
Arms     outlines   region_outlines(labels, 8) of the labels flood_regions gives (no sieve): every launch, torch's
                    scan, sort and gathers, and the host's reads of E, the rings and the vertices
         stages     device time of the entries alone: cracks (1 launch), scan (torch.cumsum), rings (2 + 2 K launches),
                    vertices (1 launch, bases made beforehand)
Device events around each sample, a warm-up of every arm first, REPEATS samples, the median reported, and its share
of the scene times DESIGN.md §17 records (16.4 ms at 1024^2, 42.8 ms at 2048^2).  Nothing here is a gate.
    python scripts/bench_outline.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flood-prediction-gan_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_regions import REPEATS, SCENE_MS, WARMUP, inputs, median_ms  # noqa: E402
from floodgan import flood_regions, ops, region_outlines  # noqa: E402
from floodgan.outline import launch_count  # noqa: E402


def spiral(R, dev):
    """logits of a one-pixel-wide spiral from the top-left corner inward, one dry pixel between its turns: straight on
    while the next pixel is free and the one after it is not flood, else one right turn, else the end"""
    m = bytearray(R * R)
    y, x, dy, dx, turned = 0, 0, 0, 1, False
    m[0] = 1
    inside = lambda v, u: 0 <= v < R and 0 <= u < R                             # noqa: E731
    while True:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and not m[ny * R + nx] and not (inside(ay, ax) and m[ay * R + ax]):
            y, x, turned = ny, nx, False
            m[y * R + x] = 1
        elif turned:
            break
        else:
            dy, dx, turned = dx, -dy, True
    mask = torch.from_numpy(np.frombuffer(bytes(m), dtype=np.uint8).reshape(R, R).copy()).to(dev)
    return torch.where(mask > 0, 4.0, -4.0)[None, None].contiguous()


def stages(labels, connectivity=8):
    H, W = labels.shape
    dev = labels.device
    sides = torch.empty((H, W), dtype=torch.uint8, device=dev)
    count = torch.empty((H, W), dtype=torch.int32, device=dev)
    out = {"cracks": median_ms(lambda: ops.outline_cracks(labels, sides, count)),
           "scan": median_ms(lambda: torch.cumsum(count.view(-1), 0, dtype=torch.int32))}
    incl = torch.cumsum(count.view(-1), 0, dtype=torch.int32)
    E = int(incl[-1])
    arr = {name: torch.empty(E, dtype=torch.int32, device=dev) for name in ("key", "ring", "edges", "corners")}
    arr["signed2"] = torch.empty(E, dtype=torch.int64, device=dev)
    arr["corner"] = torch.empty(E, dtype=torch.uint8, device=dev)
    out["rings"] = median_ms(lambda: ops.outline_rings(labels, sides, incl, connectivity, arr))
    starts = torch.nonzero(arr["ring"] == torch.arange(E, dtype=torch.int32, device=dev)).view(-1)
    corners = arr["corners"][starts].long()
    base = torch.zeros(E, dtype=torch.int32, device=dev)
    base[starts] = (torch.cumsum(corners, 0) - corners).int()
    vertices = torch.empty((int(corners.sum()), 2), dtype=torch.int32, device=dev)
    out["vertices"] = median_ms(lambda: ops.outline_vertices(arr, base, H, W, vertices))
    return out


def main():
    dev = "cuda"
    results = []
    for R, scene_ms in SCENE_MS.items():
        for name, z in list(inputs(R, dev).items()) + [("spiral", spiral(R, dev))]:
            labels = flood_regions(z, "logit", 1, 0, 8, table=False)["labels"]
            res = region_outlines(labels, 8)
            ms = median_ms(lambda: region_outlines(labels, 8))
            row = {"size": R, "input": name, "edges": res["edge_count"], "rings": res["ring_count"],
                   "vertices": res["vertex_count"], "longest_ring": int(res["rings"]["edges"].max()),
                   "launches": launch_count(res["edge_count"]),
                   "outlines": {"median_ms": ms, "share_of_scene": round(ms / scene_ms, 4)},
                   "stages_ms": stages(labels)}
            results.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({"connectivity": 8, "warmup": WARMUP, "repeats": REPEATS, "scene_ms": SCENE_MS,
                      "results": results}))


if __name__ == "__main__":
    main()
