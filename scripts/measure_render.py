"""Sheet-to-host time of the device picture route against the host route (pictures section).

One four-panel sheet of eight 512x512 samples -- input (9-channel, channels-last, as the loader yields it) |
generator output (NCHW) | attention mask | ground truth (channels-last):

  device route   the four render launches into a Canvas and its single device-to-host copy (floodgan.render)
  host route     .cpu() of the same four fp32 tensors, then the numpy rules of tests/render_oracle.py composed into
                 the same sheet -- what a user could do before floodgan.render existed

Both routes are warmed, then timed alternately (host clock around work that ends in a synchronise); medians are
reported, and the two sheets must be equal byte for byte.   python scripts/measure_render.py [--trace]
--trace runs only the device route a few times, for a kernel / copy trace taken in a run of its own.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flood-prediction-gan_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import render_oracle as RO  # noqa: E402
from floodgan.render import Canvas, sheet_layout  # noqa: E402

N, R, GUTTER = 8, 512, 8


def main():
    trace = "--trace" in sys.argv
    dev = "cuda"
    g = torch.Generator().manual_seed(47)
    x = (torch.rand((N, 9, R, R), generator=g) * 2.4 - 1.2).to(dev).contiguous(memory_format=torch.channels_last)
    out = (torch.rand((N, 3, R, R), generator=g) * 2.4 - 1.2).to(dev)
    mask = torch.rand((N, R, R), generator=g).to(dev)
    y = (torch.rand((N, 3, R, R), generator=g) * 2.4 - 1.2).to(dev).contiguous(memory_format=torch.channels_last)
    height, width, off = sheet_layout(N, 4, R, R, GUTTER)
    cv = Canvas(height, width, dev)
    step = R + GUTTER

    def device_route():
        cv.rgb(x, 0, off[0][0][1], step_rows=step)
        cv.rgb(out, 0, off[0][1][1], step_rows=step)
        cv.scalar(mask, 0, off[0][2][1], cmap="gray_r", kind="unit", step_rows=step)
        cv.rgb(y, 0, off[0][3][1], step_rows=step)
        return cv.host()

    def host_copies():
        return x.cpu(), out.cpu(), mask.cpu(), y.cpu()

    def host_compose(xc, oc, mc, yc):
        sheet = np.full((height, width, 4), 255, dtype=np.uint8)
        cols = [RO.rgb_bytes(xc[:, :3].permute(0, 2, 3, 1).numpy()), RO.rgb_bytes(oc.permute(0, 2, 3, 1).numpy()),
                RO.scalar_bytes(mc.numpy(), "gray_r", "unit"), RO.rgb_bytes(yc.permute(0, 2, 3, 1).numpy())]
        for c, panels in enumerate(cols):
            for r in range(N):
                r0, c0 = off[r][c]
                sheet[r0:r0 + R, c0:c0 + R] = panels[r]
        return sheet

    if trace:
        for _ in range(10):
            device_route()
        torch.cuda.synchronize()
        print("traced 10 device-route sheets")
        return
    for _ in range(5):
        a = device_route().copy()
        b = host_compose(*host_copies())
    assert np.array_equal(a, b), "the two routes disagree"
    t_dev, t_copy, t_np = [], [], []
    for _ in range(30):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device_route()
        t1 = time.perf_counter()
        hc = host_copies()
        t2 = time.perf_counter()
        host_compose(*hc)
        t3 = time.perf_counter()
        t_dev.append(t1 - t0)
        t_copy.append(t2 - t1)
        t_np.append(t3 - t2)

    def ms(v):
        return {"median_ms": round(statistics.median(v) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3),
                "max_ms": round(max(v) * 1e3, 3)}
    fp32_bytes = sum(t.numel() * 4 for t in (x, out, mask, y))
    print(json.dumps({"sheet": [height, width], "samples": N, "resolution": R, "repeats": 30,
                      "sheet_bytes": int(cv._host.numel()), "fp32_bytes": fp32_bytes,
                      "device_route_render_plus_copy": ms(t_dev), "host_route_four_cpu_copies": ms(t_copy),
                      "host_route_numpy_rules": ms(t_np),
                      "host_route_total": ms([a + b for a, b in zip(t_copy, t_np)]), "sheets_equal": True}))


if __name__ == "__main__":
    main()
