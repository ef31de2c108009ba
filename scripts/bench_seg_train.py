"""Segmentation-model training step, this path vs stock PyTorch-ROCm, on one MI355X ("Training the
segmentation U-Net").  Both arms run the identical step -- UNet(3, 1) forward in training mode, BCEWithLogitsLoss,
backward, Adam(1e-4, (0.5, 0.999)) -- in one process on the same box: arm A is floodgan's fused SegStep (libfloodgan
kernels), arm B the same network from torch.nn modules (MIOpen convolutions, ATen BatchNorm / pool / loss,
torch.optim.Adam).  After warm-up the arms alternate in rounds of `--chunk` steps, each round timed with HIP events;
the figure per arm is the median round.  Measurement infrastructure only -- not the product path.
  python scripts/bench_seg_train.py [--batch 1] [--res 1024] [--steps 24] [--warmup 3] [--chunk 4]
  python scripts/bench_seg_train.py --arm hip --steps 3        (one arm alone: the form a kernel profiler wraps)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flood-prediction-gan_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402


def stock_unet():
    """models/model_architectures.py:508-587 restated from torch.nn (bilinear=False; H, W multiples of 16)"""

    def dc(i, o):
        return nn.Sequential(nn.Conv2d(i, o, 3, padding=1, bias=False), nn.BatchNorm2d(o), nn.ReLU(inplace=True),
                             nn.Conv2d(o, o, 3, padding=1, bias=False), nn.BatchNorm2d(o), nn.ReLU(inplace=True))

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            ch = [64, 128, 256, 512, 1024]
            self.enc = nn.ModuleList([dc(3, 64)] + [dc(ch[k - 1], ch[k]) for k in range(1, 5)])
            self.up = nn.ModuleList([nn.ConvTranspose2d(ch[k], ch[k - 1], 2, 2) for k in range(4, 0, -1)])
            self.dec = nn.ModuleList([dc(ch[k], ch[k - 1]) for k in range(4, 0, -1)])
            self.outc = nn.Conv2d(64, 1, 1)
            self.pool = nn.MaxPool2d(2)

        def forward(self, x):
            skips = []
            for k, e in enumerate(self.enc):
                x = e(self.pool(x) if k else x)
                skips.append(x)
            for i, (u, d) in enumerate(zip(self.up, self.dec)):
                x = d(torch.cat([skips[3 - i], u(x)], dim=1))
            return self.outc(x)

    return Net()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=24, help="timed steps per arm")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=4, help="steps per timed round; the arms alternate by round")
    ap.add_argument("--arm", choices=["both", "hip", "stock"], default="both")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_train needs a HIP device: there is no CPU measurement path")
    from floodgan.segmentation import SegmentationModel, SegStep
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(77)
    x = torch.rand((a.batch, 3, a.res, a.res), generator=g).to(dev)
    t = (torch.rand((a.batch, 1, a.res, a.res), generator=g) > 0.6).float().to(dev)
    torch.manual_seed(5)
    arms = {}
    if a.arm in ("both", "hip"):
        m = SegmentationModel(train=True, device="cuda", verbose=False)
        m.model.train()
        last = {}

        def hip_step():
            last["hip"] = m.step_fn(x, t)

        arms["hip"] = hip_step
    if a.arm in ("both", "stock"):
        net = stock_unet().to(dev).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.5, 0.999))
        crit = nn.BCEWithLogitsLoss()

        def stock_step():
            loss = crit(net(x), t)
            opt.zero_grad()
            loss.backward()
            opt.step()

        arms["stock"] = stock_step
    for fn in arms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in arms}
    for _ in range(-(-a.steps // a.chunk)):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.chunk):
                fn()
            e1.record()
            e1.synchronize()
            rounds[name].append(e0.elapsed_time(e1) / a.chunk)
    out = {"what": "segmentation training step, HIP-event timed, arms alternating in rounds", "batch": a.batch,
           "res": a.res, "steps_per_arm": len(next(iter(rounds.values()))) * a.chunk, "chunk": a.chunk,
           "torch": torch.__version__}
    for name, ms in rounds.items():
        med = statistics.median(ms)
        out[name] = {"ms_per_step_median": round(med, 3), "ms_per_step_min": round(min(ms), 3),
                     "ms_per_step_max": round(max(ms), 3), "img_per_s": round(1e3 * a.batch / med, 3)}
    if len(arms) == 2:
        out["ratio_hip_over_stock_img_per_s"] = round(out["hip"]["img_per_s"] / out["stock"]["img_per_s"], 4)
    if "hip" in arms:
        loss, acc = SegStep.read(last["hip"], t.numel())
        out["hip_last_loss_accuracy"] = [round(loss, 5), round(acc, 5)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
