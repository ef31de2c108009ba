"""Time and peak memory of the flood-mask loss at 512x512, batch 8, eval-mode statistics.

  A        floodgan.FloodMaskLoss forward + backward to the image (frozen U-Net: save="input", param_grads=False)
  A_full   the same pieces with the full saved state and every parameter gradient (save=True, param_grads=True):
           what skipping the weight gradients and their operands saves
  B        the same computation by stock PyTorch-ROCm in fp32: the functional restatement of the U-Net
           (tests/seg_train_oracle.py) on the device, frozen parameters, autograd to the image

The arms are warmed, then timed alternately, 30 repeats, a host clock around work that ends in a synchronise (the
protocol of scripts/measure_render.py); medians and ranges are reported, and each arm's peak allocation
(torch.cuda.max_memory_allocated over one call, above what was allocated before it).
    python scripts/bench_flood_mask_loss.py [--trace]
--trace runs only arm A a few times, for a kernel trace taken in a run of its own.
"""
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flood-prediction-gan_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import seg_train_oracle as SO  # noqa: E402
from floodgan import FloodMaskLoss, ops  # noqa: E402
from floodgan import segmentation as S  # noqa: E402
from floodgan.plans import Buf  # noqa: E402

N, R, REPEATS = 8, 512, 30


def main():
    trace = "--trace" in sys.argv
    dev = "cuda"
    torch.manual_seed(47)
    net = S.UNet().apply(S.initialise_weights).to(dev)
    g = torch.Generator().manual_seed(48)
    with torch.no_grad():
        for k, b in net.named_buffers():                   # running statistics away from (0, 1)
            if k.endswith("running_mean"):
                b.add_((torch.randn(b.shape, generator=g) * 0.05).to(dev))
            elif k.endswith("running_var"):
                b.mul_((0.5 + torch.rand(b.shape, generator=g)).to(dev))
    loss = FloodMaskLoss(net)
    fake = (torch.rand((N, 3, R, R), generator=g) * 2.4 - 1.2).to(dev)
    real = (torch.rand((N, 3, R, R), generator=g) * 2.4 - 1.2).to(dev)
    P, B = dict(net.named_parameters()), dict(net.named_buffers())
    Pd = {k: v.detach() for k, v in P.items()}

    def arm_a():
        x = fake.detach().requires_grad_(True)
        loss(x, real).backward()
        return x.grad

    def arm_a_full():
        with torch.no_grad():
            F0, R0 = S.unit_image(fake, buf=True, nchw=False)[1], S.unit_image(real, buf=True, nchw=False)[1]
            r = S.unet_logits(P, B, R0, False)
            z, saved = S.unet_logits(P, B, F0, False, save=True)
            res = torch.empty(2, dtype=torch.int64, device=dev)
            gz = Buf.empty(N, R, R, 4, 0, dev)
            ops.flood_mask_bce(z, r, 1.0 / (N * R * R), gz, res)
            grads = S.unet_backward(P, saved, gz, input_grad=True)
            out = torch.empty_like(fake)
            ops.unit_image_bwd(grads["input"], fake, out)
        return out

    def arm_b():
        x = fake.detach().requires_grad_(True)
        with torch.no_grad():
            t = (torch.sigmoid(SO.unet_forward(Pd, B, torch.clamp((real + 1) * 0.5, 0, 1), False)) > 0.5).float()
        z = SO.unet_forward(Pd, B, torch.clamp((x + 1) * 0.5, 0, 1), False)
        F.binary_cross_entropy_with_logits(z, t).backward()
        return x.grad

    if trace:
        for _ in range(5):
            arm_a()
        torch.cuda.synchronize()
        print("traced 5 FloodMaskLoss forward + backward calls")
        return
    arms = {"A_flood_mask_loss": arm_a, "A_full_param_grads": arm_a_full, "B_stock_pytorch_fp32": arm_b}
    outs, peak = {}, {}
    for name, fn in arms.items():
        for _ in range(3):
            outs[name] = fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    ga, gb = outs["A_flood_mask_loss"].double(), outs["B_stock_pytorch_fp32"].double()
    assert torch.equal(outs["A_flood_mask_loss"], outs["A_full_param_grads"])
    times = {name: [] for name in arms}
    for _ in range(REPEATS):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)

    def ms(v):
        return {"median_ms": round(statistics.median(v) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3),
                "max_ms": round(max(v) * 1e3, 3)}
    print(json.dumps({"batch": N, "resolution": R, "repeats": REPEATS, "statistics": "eval",
                      **{name: {**ms(v), "peak_MiB": round(peak[name] / 2 ** 20, 1)} for name, v in times.items()},
                      "A_vs_B_gradient_nrel": float((ga - gb).norm() / gb.norm())}))


if __name__ == "__main__":
    main()
