"""Evaluation inference on the HIP path: the segmentation U-Net vs the
reference's own UNet (golden) and the fp64 oracle, the metric kernels vs the oracle's torchmetrics-1.2.0
restatement (formula parity unpinned: torchmetrics is absent), and calculate_metrics end to end."""
import os

import numpy as np
import pytest
import torch

from oracle import evaluation as OE
from test_gpu_parity import DEV, nrel

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmentation_unet_64.npz")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _unet():
    from floodgan.segmentation import UNet, initialise_weights
    torch.manual_seed(5)
    return UNet().apply(initialise_weights)


def test_unet_vs_reference_golden(report):
    gold = {k.replace("__", "."): v for k, v in np.load(GOLD).items()}
    net = _unet().to(DEV)
    g = torch.Generator().manual_seed(77)
    x1 = torch.rand((2, 3, 64, 64), generator=g)
    with torch.no_grad():
        logits = net(x1.to(DEV))
    ref = torch.from_numpy(gold["logits_64"])
    e = nrel(logits, ref)
    agree = float(((logits.cpu() > 0) == (ref > 0)).double().mean())
    report("segmentation_unet_vs_golden", logits_rel=e, mask_agreement=agree)
    assert e < 1e-4 and agree > 0.999
    # training-mode BatchNorm: the running statistics moved exactly as the reference's first call
    net_c = _unet()
    P = dict(net_c.named_parameters())
    B = {k: v.clone() for k, v in net_c.named_buffers()}
    with torch.no_grad():
        OE.unet_forward(P, B, x1)
    worst = max(nrel(v, B[k]) for k, v in net.named_buffers() if v.is_floating_point())
    assert worst < 1e-5, worst


@pytest.mark.parametrize("n,res", [(1, 256), (3, 192), (2, 512)])
def test_metric_kernels_vs_oracle(n, res, report):
    from floodgan.evaluate import ImageMetrics
    g = torch.Generator().manual_seed(res + n)
    a = torch.rand((n, 3, res, res), generator=g)
    b = (a + 0.15 * torch.randn(a.shape, generator=g)).clamp(0, 1)
    im = ImageMetrics(DEV)
    ad, bd = a.to(DEV), b.to(DEV)
    got = dict(psnr=im.psnr(ad, bd), ssim=im.ssim(ad, bd), ms_ssim=im.ms_ssim(ad, bd))
    ref = dict(psnr=OE.psnr(a, b), ssim=OE.ssim(a, b), ms_ssim=OE.ms_ssim(a, b))
    report("metric_kernels_vs_oracle", n=n, res=res, got=got, ref=ref)
    assert abs(got["psnr"] - ref["psnr"]) < 1e-6 * abs(ref["psnr"])
    assert abs(got["ssim"] - ref["ssim"]) < 2e-6
    assert abs(got["ms_ssim"] - ref["ms_ssim"]) < 2e-6
    assert im.ssim(ad, ad) == pytest.approx(1.0, abs=1e-6)


def test_mask_confusion_vs_oracle():
    from floodgan.evaluate import MaskConfusion
    from floodgan.plans import Buf
    g = torch.Generator().manual_seed(9)
    lp, lt = torch.randn(2, 1, 40, 48, generator=g), torch.randn(2, 1, 40, 48, generator=g)
    bufs = []
    for t in (lp, lt):
        b = Buf.zeros(2, 40, 48, 4, 0, DEV)
        b.interior()[..., 0] = t[:, 0].to(DEV)
        bufs.append(b)
    mc = MaskConfusion(DEV)
    mc.update(*bufs)
    mc.update(*bufs)                                   # accumulates like the reference's torch.cat
    got = mc.compute()
    ref = OE.binary_metrics(torch.cat([OE.flood_mask(lp)] * 2), torch.cat([OE.flood_mask(lt)] * 2))
    assert all(got[k] == pytest.approx(ref[k], abs=1e-12) for k in ref), (got, ref)


def test_calculate_metrics_end_to_end(report):
    """Model.calculate_metrics on a synthetic two-batch loader at 256x256 (PairedAttention, seed-47
    weights) vs the same pipeline with the oracle's metrics and UNet (fp64) on the HIP generator outputs"""
    from floodgan.model import Model
    from floodgan.segmentation import UNet, initialise_weights
    g = torch.Generator().manual_seed(21)
    batches = [(torch.rand((2, 9, 256, 256), generator=g) * 2 - 1, torch.rand((2, 3, 256, 256), generator=g) * 2 - 1,
                ["hurricane-harvey_0", "hurricane-harvey_1"]) for _ in range(2)]
    m = Model(model="PairedAttention", training_model=False, val_loader=batches, device=DEV)
    torch.manual_seed(5)
    seg = UNet().apply(initialise_weights)
    seg_ref = {k: v.detach().double().clone() for k, v in seg.state_dict().items()}
    df = m.calculate_metrics(seg_model=seg.to(DEV))
    got = df.iloc[0].to_dict()
    # oracle pipeline on the same generator outputs
    P = {k: v for k, v in seg_ref.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    B = {k: v for k, v in seg_ref.items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    per = {"PSNR": [], "SSIM": [], "MS-SSIM": []}
    pm, tm = [], []
    for x, y, _ in batches:
        torch.manual_seed(47)
        with torch.no_grad():
            out = m.generator(x.to(DEV)).cpu().double()
        go, gt = OE.unit_image(out), OE.unit_image(y.double())
        per["PSNR"].append(OE.psnr(go, gt))
        per["SSIM"].append(OE.ssim(go, gt))
        per["MS-SSIM"].append(OE.ms_ssim(go, gt))
        with torch.no_grad():
            pm.append(OE.flood_mask(OE.unet_forward(P, B, go)))
            tm.append(OE.flood_mask(OE.unet_forward(P, B, gt)))
    ref = {k: float(np.mean(v)) for k, v in per.items()}
    ref.update(OE.binary_metrics(torch.cat(pm), torch.cat(tm)))
    report("calculate_metrics_end_to_end", got={k: float(v) for k, v in got.items()}, ref=ref)
    for k in ("PSNR", "SSIM", "MS-SSIM"):
        assert abs(got[k] - ref[k]) < 1e-5 * max(1.0, abs(ref[k])), (k, got[k], ref[k])
    # masks: a logit within rounding of 0 may land on either side -> 1e-3 of the pixels
    for k in ("MSE", "Accuracy", "F1_Flood", "Precision_Flood", "Recall_Flood", "F1_No_Flood", "Precision_No_Flood",
              "Recall_No_Flood"):
        assert abs(got[k] - ref[k]) < 1e-3, (k, got[k], ref[k])
    assert np.isnan(got["LPIPS"]) and got["Inference"] > 0


# ------------------------------------------------------------------ metric kernels at their edges
#
# The kernels are fp32 by design, as torchmetrics is, so each case's tolerance is measured from the oracle
# itself: max(2e-6, 4 x |oracle run in float32 - oracle in float64|), the factor 4 covering a different
# summation order.  Each tolerance is also held below a tenth of what shifting `b` by one pixel changes.

def _noise_pair(n, h, w):
    g = torch.Generator().manual_seed(1000 * n + 7 * h + w)
    a = torch.rand((n, 3, h, w), generator=g)
    b = (a + 0.15 * torch.randn(a.shape, generator=g)).clamp(0, 1)
    return a, b


def _smooth_pair(h, w):
    """bright, low-variance images of different structure: sigma^2 = E[x^2] - mu^2 cancels in fp32"""
    y = torch.arange(h, dtype=torch.float64).view(h, 1)
    x = torch.arange(w, dtype=torch.float64).view(1, w)
    a = 0.9 + 0.05 * torch.sin(x / 7) * torch.cos(y / 5)
    b = 0.88 + 0.06 * torch.cos(x / 4 + 0.5) * torch.sin(y / 6) + 0.02 * torch.sin((x + y) / 3)
    return a.float().expand(1, 3, h, w).contiguous(), b.float().expand(1, 3, h, w).contiguous()


def _oracle_with_tolerance(fn, a, b):
    """(float64 oracle value, tolerance, fp32 spread) of OE.ssim / OE.ms_ssim on fp32 CPU images"""
    ref = fn(a.double(), b.double())
    spread = abs(fn(a, b, dtype=torch.float32) - ref)
    tol = max(2e-6, 4 * spread)
    shifted = abs(fn(a.double(), torch.roll(b, 1, -1).double()) - ref)
    assert tol < 0.1 * shifted, (tol, shifted)
    return ref, tol, spread


SSIM_CASES = [("noise", 2, 11, 11),         # a single window
              ("noise", 1, 12, 27), ("noise", 2, 27, 12),
              ("noise", 3, 43, 59),         # partial 16 x 16 tiles in both axes, h != w, 3 x 4 tiles
              ("smooth", 1, 43, 59)]


@pytest.mark.parametrize("kind,n,h,w", SSIM_CASES)
def test_ssim_shapes_vs_oracle(kind, n, h, w, report):
    from floodgan.evaluate import ImageMetrics
    a, b = _noise_pair(n, h, w) if kind == "noise" else _smooth_pair(h, w)
    ref, tol, spread = _oracle_with_tolerance(OE.ssim, a, b)
    im = ImageMetrics(DEV)
    ad, bd = a.to(DEV), b.to(DEV)
    got = im.ssim(ad, bd)
    print(f"ssim {kind} {(n, h, w)}: got {got!r} ref {ref!r} err {abs(got - ref):.2e} tol {tol:.2e} "
          f"(fp32 spread {spread:.2e})")
    report("ssim_shapes_vs_oracle", kind=kind, shape=[n, h, w], err=abs(got - ref), tol=tol, spread=spread)
    assert abs(got - ref) < tol
    # per image, and the contrast-sensitivity mean, against the oracle's per-image values
    s_ref, cs_ref = OE._ssim_and_cs(a.double(), b.double())
    s_32, cs_32 = OE._ssim_and_cs(a, b, dtype=torch.float32)
    tol_i = max(2e-6, 4 * float((s_32 - s_ref).abs().max()), 4 * float((cs_32 - cs_ref).abs().max()))
    s_got, cs_got = im._ssim_cs(ad, bd, want_cs=True)
    err_i = max(float((s_got.cpu() - s_ref).abs().max()), float((cs_got.cpu() - cs_ref).abs().max()))
    print(f"  per image (ssim, cs): err {err_i:.2e} tol {tol_i:.2e}")
    assert err_i < tol_i
    # a against itself: the oracle gives exactly 1 in either dtype (no spread), so the rule's floor applies.  The
    # kernel's sab - ma * mb and saa - ma^2 may contract to FMAs differently, which the cancellation of a
    # low-variance image magnifies
    self_err = abs(im.ssim(ad, ad) - 1.0)
    print(f"  ssim(a, a) - 1: {self_err:.2e}")
    assert OE.ssim(a, a, dtype=torch.float32) == 1.0 == OE.ssim(a.double(), a.double())
    assert self_err < 2e-6


MS_SSIM_SHAPES = [(2, 177, 203),            # odd sizes: every halving drops a row or a column
                  (1, 176, 176),            # the last scale is one 11 x 11 window
                  (1, 191, 176)]            # 191 -> 95 -> 47 -> 23 -> 11, 176 -> 11


@pytest.mark.parametrize("n,h,w", MS_SSIM_SHAPES)
def test_ms_ssim_shapes_vs_oracle(n, h, w, report):
    from floodgan.evaluate import ImageMetrics
    a, b = _noise_pair(n, h, w)
    ref, tol, spread = _oracle_with_tolerance(OE.ms_ssim, a, b)
    im = ImageMetrics(DEV)
    got = im.ms_ssim(a.to(DEV), b.to(DEV))
    print(f"ms_ssim {(n, h, w)}: got {got!r} ref {ref!r} err {abs(got - ref):.2e} tol {tol:.2e} "
          f"(fp32 spread {spread:.2e})")
    report("ms_ssim_shapes_vs_oracle", shape=[n, h, w], err=abs(got - ref), tol=tol, spread=spread)
    assert abs(got - ref) < tol


def test_ms_ssim_relu_clamp():
    """b = 1 - a: cs is about -0.99 at every scale, relu clamps it and the product is exactly 0"""
    from floodgan.evaluate import ImageMetrics
    a, _ = _noise_pair(2, 177, 203)
    im = ImageMetrics(DEV)
    ad = a.to(DEV)
    bd = 1 - ad
    _, cs = im._ssim_cs(ad, bd, want_cs=True)
    assert float(cs.max()) < -0.9
    assert im.ms_ssim(ad, bd) == 0.0 == OE.ms_ssim(a.double(), 1 - a.double())
    bd[1] = ad[1]                                    # image 1 identical -> 1, image 0 clamped -> 0
    assert abs(im.ms_ssim(ad, bd) - 0.5) < 1e-6


@pytest.mark.parametrize("h,w", [(191, 161), (161, 191)])
def test_ms_ssim_rejects_small_side(h, w):
    """torchmetrics applies its size rule (side // 16 > 10) to both sides"""
    from floodgan.evaluate import ImageMetrics
    im = ImageMetrics(DEV)
    x = torch.rand(1, 3, h, w, device=DEV)
    with pytest.raises(ValueError):
        im.ms_ssim(x, x)
    ok = torch.rand(1, 3, 176, 191, device=DEV)
    assert im.ms_ssim(ok, ok) == pytest.approx(1.0, abs=1e-6)


@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (2, 37, 53)])
def test_unit_image_strided_both_outputs(n, h, w):
    """fg_unit_image from a channels-last channel slice into the NCHW tensor and a bordered 4-channel Buf at
    once: bit-exact with torch.clamp((x + 1) * 0.5, 0, 1) in fp32; border and channel 3 untouched"""
    from floodgan.plans import Buf
    from floodgan.segmentation import unit_image
    g = torch.Generator().manual_seed(h + w)
    x9 = torch.randn((n, 9, h, w), generator=g)
    special = torch.tensor([-1.0, 1.0, 1.5, -1.5, 1e-8, -1e-8, 0.0, -0.0, 0.99999994, -0.99999994])
    x9[0, 2:5].view(-1)[:special.numel()] = special
    x9[n - 1, 4].view(-1)[-special.numel():] = special
    xd = x9.to(DEV).contiguous(memory_format=torch.channels_last)
    src = xd[:, 2:5]
    assert src.stride() == (9 * h * w, 1, 9 * w, 9) and src.data_ptr() != xd.data_ptr()
    want = torch.clamp((x9[:, 2:5] + 1) * 0.5, 0, 1)
    assert want.dtype == torch.float32 and float(want.min()) == 0.0 and float(want.max()) == 1.0
    canary = Buf(torch.full((n * (h + 2) * (w + 2) * 4,), float("nan"), device=DEV), n, h, w, 4, 1)
    out, buf = unit_image(src, buf=canary)
    torch.cuda.synchronize()
    assert buf is canary and out.is_contiguous() and torch.equal(out.cpu(), want)
    assert torch.equal(buf.interior()[..., :3].permute(0, 3, 1, 2).cpu(), want)
    full = buf.nhwc().cpu()
    assert bool(torch.isnan(full[..., 3]).all())
    border = torch.ones(n, h + 2, w + 2, dtype=torch.bool)
    border[:, 1:-1, 1:-1] = False
    assert bool(torch.isnan(full[border]).all())
    # one output at a time gives the same bits
    only_nchw, none = unit_image(src, buf=None)
    assert none is None and torch.equal(only_nchw.cpu(), want)
    no_nchw, buf2 = unit_image(src, buf=True, nchw=False)
    assert no_nchw is None and torch.equal(buf2.interior()[..., :3].permute(0, 3, 1, 2).cpu(), want)
    assert float(buf2.nhwc()[..., 3].abs().max()) == 0.0
    assert torch.equal(xd.cpu(), x9)


@pytest.mark.parametrize("planes,h,w", [(5, 7, 9), (3, 2, 2)])
def test_avg_pool2_vs_fp64(planes, h, w):
    """F.avg_pool2d(x, 2): odd sizes drop the last row / column"""
    import torch.nn.functional as F
    from floodgan import _lib as L
    g = torch.Generator().manual_seed(planes * h + w)
    x = torch.rand((planes, h, w), generator=g)
    ref = F.avg_pool2d(x.double().unsqueeze(0), 2)[0]
    total = ref.numel()
    assert ref.shape == (planes, h // 2, w // 2)
    dst = torch.full((total + 8,), float("nan"), device=DEV)
    xd = x.to(DEV)
    L.check(L.load().fg_avg_pool2(L.ptr(xd), planes, h, w, L.ptr(dst), L.stream_handle()), "avg_pool2")
    torch.cuda.synchronize()
    got = dst[:total].cpu().double().view_as(ref)
    assert float((got - ref).abs().max()) < 1e-6 * float(ref.abs().max())
    assert bool(torch.isnan(dst[total:]).all()) and torch.equal(xd.cpu(), x)


def test_psnr_identical_and_small_difference():
    from floodgan.evaluate import ImageMetrics
    g = torch.Generator().manual_seed(19)
    a = torch.rand((1, 3, 11, 13), generator=g) * 0.99
    b = a + 1.0 / 255
    im = ImageMetrics(DEV)
    ad, bd = a.to(DEV), b.to(DEV)
    assert im.psnr(ad, ad) == float("inf")
    ref = OE.psnr(a.double(), b.double())
    assert 48.0 < ref < 48.3                          # 20 log10(255) = 48.13
    assert abs(im.psnr(ad, bd) - ref) < 1e-6 * ref


def _logit_buf(logits, pad, gen):
    """4-channel Buf with `logits` [N, H, W] in channel 0, NaN in the border, garbage in channels 1-3"""
    from floodgan.plans import Buf
    n, h, w = logits.shape
    t = torch.full((n, h + 2 * pad, w + 2 * pad, 4), float("nan"))
    t[:, pad:pad + h, pad:pad + w, 0] = logits
    t[:, pad:pad + h, pad:pad + w, 1:] = -1e3 * torch.sign(logits).unsqueeze(-1) * \
        torch.rand((n, h, w, 3), generator=gen)
    return Buf(t.reshape(-1).to(DEV), n, h, w, 4, pad)


@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (3, 512, 512)])      # the second: past 2048 blocks x 256 threads
def test_mask_confusion_counts(n, h, w):
    """tp / fp / tn / fn are the integer counts of logit > 0 for |logit| >= 2^-20 (inside that band sigmoid
    rounds to 0.5 in fp32 and either side is legitimate), saturating and infinite logits included; the views
    differ in their border width"""
    from floodgan.evaluate import MaskConfusion
    g = torch.Generator().manual_seed(n * h + w)
    tiny = 2.0 ** -20
    special = torch.tensor([88.0, -88.0, 104.0, -104.0, float("inf"), float("-inf"), tiny, -tiny])
    logits = []
    for k in range(2):
        z = torch.randn((n, h, w), generator=g) * (0.01 if k else 1.0)
        z = torch.where(z.abs() < tiny, torch.full_like(z, tiny) * torch.where(z < 0, -1.0, 1.0), z)
        flat = z.view(-1)
        flat[k:k + 8] = special                       # offset by one: every pairing of signs occurs
        flat[-8 - k:flat.numel() - k] = special
        assert float(z.abs().min()) >= tiny
        logits.append(z)
    lp, lt = logits
    mc = MaskConfusion(DEV)
    mc.update(_logit_buf(lp, 1, g), _logit_buf(lt, 2, g))
    got = [int(v) for v in mc.counts.cpu()]
    p, t = lp > 0, lt > 0
    want = [int((p & t).sum()), int((p & ~t).sum()), int((~p & ~t).sum()), int((~p & t).sum())]
    assert got == want and sum(got) == n * h * w and min(want) > 0
    assert torch.equal(p, OE.flood_mask(lp.double()) > 0) and torch.equal(t, OE.flood_mask(lt.double()) > 0)


def test_mask_confusion_zero_is_no_flood():
    """sigmoid(+-0) = 0.5 is not > 0.5: both zeros are no-flood, as torch.sigmoid(x) > 0.5"""
    from floodgan.evaluate import MaskConfusion
    g = torch.Generator().manual_seed(2)
    z = torch.zeros(1, 3, 4)
    z.view(-1)[::2] = -0.0
    assert not bool((torch.sigmoid(z) > 0.5).any())
    ones = torch.ones(1, 3, 4)
    mc = MaskConfusion(DEV)
    mc.update(_logit_buf(z, 1, g), _logit_buf(-z, 2, g))
    assert [int(v) for v in mc.counts.cpu()] == [0, 0, 12, 0]
    mc.update(_logit_buf(z, 1, g), _logit_buf(ones, 2, g))
    assert [int(v) for v in mc.counts.cpu()] == [0, 0, 12, 12]
