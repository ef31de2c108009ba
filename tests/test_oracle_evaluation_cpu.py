"""The evaluation oracle (oracle/evaluation.py) and the segmentation drop-in modules on the CPU: the
reference UNet's golden (tests/golden/make_golden_segmentation.py), and the metric restatements'
known-answer properties (torchmetrics is absent: formula parity unpinned)."""
import os

import numpy as np
import pytest
import torch

from oracle import evaluation as OE

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmentation_unet_64.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k.replace("__", "."): z[k] for k in z.files}


def _ours():
    from floodgan.segmentation import UNet, initialise_weights
    torch.manual_seed(5)
    return UNet().apply(initialise_weights)


def test_unet_modules_match_reference_init(gold):
    net = _ours()
    keys = [k[len("init/"):] for k in gold if k.startswith("init/")]
    assert list(net.state_dict()) == keys
    for name, t in net.state_dict().items():
        ref = gold["init/" + name]
        t = t.double().flatten()
        n8 = min(8, t.numel())
        assert np.array_equal(t[:n8].numpy(), ref[2:2 + n8]), name
        assert abs(t.sum().item() - ref[0]) <= 1e-9 * max(1.0, abs(ref[1])), name


def test_oracle_unet_matches_reference_golden(gold):
    net = _ours()
    P = dict(net.named_parameters())
    B = {k: v.clone() for k, v in net.named_buffers()}
    g = torch.Generator().manual_seed(77)
    x1 = torch.rand((2, 3, 64, 64), generator=g)
    x2 = torch.rand((1, 3, 48, 48), generator=g)
    with torch.no_grad():
        l1 = OE.unet_forward(P, B, x1)
        l2 = OE.unet_forward(P, B, x2)
    for out, ref in ((l1, gold["logits_64"]), (l2, gold["logits_48"])):
        assert np.linalg.norm(out.numpy() - ref) / np.linalg.norm(ref) < 1e-5
    for k, v in B.items():
        if not v.is_floating_point():
            continue
        ref = gold["after/" + k]
        assert abs(v.double().sum().item() - ref[0]) <= 1e-4 * max(1.0, abs(ref[1])), k


def test_metric_restatements_known_answers():
    g = torch.Generator().manual_seed(3)
    a = torch.rand((2, 3, 192, 192), generator=g, dtype=torch.float64)
    assert OE.ssim(a, a) == pytest.approx(1.0, abs=1e-12)
    assert OE.ms_ssim(a, a) == pytest.approx(1.0, abs=1e-12)
    b = (a + 0.1).clamp(0, 1)
    mse = float(((a - b) ** 2).mean())
    assert OE.psnr(a, b) == pytest.approx(10 * np.log10(1 / mse), rel=1e-12)
    # SSIM on a constant shift: luminance term only changes; structure intact -> close to but below 1
    s = OE.ssim(a, b)
    assert 0.5 < s < 1.0
    # windows: the cropped map covers exactly the windows inside the image
    s1, cs1 = OE._ssim_and_cs(a[:, :, :64, :64], b[:, :, :64, :64])
    assert s1.shape == (2,) and cs1.shape == (2,)


def test_binary_metrics_restatement():
    p = torch.tensor([1, 1, 0, 0, 1, 0, 1, 0], dtype=torch.float32)
    t = torch.tensor([1, 0, 0, 1, 1, 0, 0, 0], dtype=torch.float32)
    m = OE.binary_metrics(p, t)
    tp, fp, fn, tn = 2, 2, 1, 3
    assert m["MSE"] == pytest.approx((fp + fn) / 8)
    assert m["Accuracy"] == pytest.approx((tp + tn) / 8)
    assert m["Precision_Flood"] == pytest.approx(tp / (tp + fp))
    assert m["Recall_Flood"] == pytest.approx(tp / (tp + fn))
    assert m["F1_Flood"] == pytest.approx(2 * tp / (2 * tp + fp + fn))
    assert m["Precision_No_Flood"] == pytest.approx(tn / (tn + fn))
    assert m["Recall_No_Flood"] == pytest.approx(tn / (tn + fp))
    # zero division -> 0 (torchmetrics' _safe_divide)
    z = OE.binary_metrics(torch.zeros(4), torch.zeros(4))
    assert z["Precision_Flood"] == 0.0 and z["F1_Flood"] == 0.0 and z["Accuracy"] == 1.0


def test_evaluate_host_helpers():
    """the device path's host arithmetic: the gaussian window and the confusion-count metrics"""
    from floodgan.evaluate import MaskConfusion, extract_input_topography, gaussian11
    g = gaussian11()
    assert g.dtype == torch.float32 and abs(float(g.sum()) - 1) < 1e-6 and g.argmax() == 5
    assert torch.allclose(g.double(), OE._gaussian().flatten(), atol=1e-7)
    mc = MaskConfusion(device="cpu")
    mc.counts = torch.tensor([2, 2, 3, 1])            # tp, fp, tn, fn of test_binary_metrics_restatement
    p = torch.tensor([1, 1, 0, 0, 1, 0, 1, 0], dtype=torch.float32)
    t = torch.tensor([1, 0, 0, 1, 1, 0, 0, 0], dtype=torch.float32)
    ref = OE.binary_metrics(p, t)
    got = mc.compute()
    assert all(got[k] == pytest.approx(ref[k]) for k in ref)
    x = torch.arange(9.0).view(1, 9, 1, 1)
    assert extract_input_topography(x, "flow").flatten().tolist() == [0, 1, 2, 4]
    assert extract_input_topography(x, None).flatten().tolist() == [0, 1, 2]
    assert extract_input_topography(x[:, :4], "dem").shape[1] == 4
    with pytest.raises(ValueError):
        extract_input_topography(x[:, :5], "map")


# ------------------------------------------------------------------ the metric formulas, pinned by closed forms
#
# torchmetrics is absent, so the restatements are held to what the published SSIM definition gives in closed
# form: with a normalised window, constant images have zero windowed (co)variance, and b = s * a has
# sigma_b^2 = s^2 sigma_a^2, sigma_ab = s sigma_a^2.

C1, C2 = 0.01 ** 2, 0.03 ** 2


def test_gaussian_window_closed_form():
    g = OE._gaussian().flatten()
    assert g.dtype == torch.float64 and g.numel() == 11
    assert torch.equal(g, g.flip(0))
    assert float(g.sum()) == pytest.approx(1.0, abs=1e-15)
    for i in range(10):
        k = i - 5                                    # tap offsets -5 .. 5: g(k + 1) / g(k)
        assert float(g[i + 1] / g[i]) == pytest.approx(np.exp(-(2 * k + 1) / (2 * 1.5 ** 2)), rel=1e-12)
    g32 = OE._gaussian(dtype=torch.float32)
    assert g32.dtype == torch.float32 and torch.allclose(g32.double().flatten(), g, atol=1e-7)


@pytest.mark.parametrize("alpha,beta", [(0.3, 0.3), (0.2, 0.9), (0.0, 1.0), (0.5, 0.0)])
def test_ssim_constant_images_closed_form(alpha, beta):
    a = torch.full((2, 3, 17, 23), alpha, dtype=torch.float64)
    b = torch.full((2, 3, 17, 23), beta, dtype=torch.float64)
    s, cs = OE._ssim_and_cs(a, b)
    want = (2 * alpha * beta + C1) / (alpha ** 2 + beta ** 2 + C1)
    assert s.shape == (2,) and float((s - want).abs().max()) < 1e-9
    assert float((cs - 1.0).abs().max()) < 1e-9
    assert OE.ssim(a, b) == pytest.approx(want, abs=1e-9)


@pytest.mark.parametrize("s", [0.25, 0.6, 1.0])
def test_cs_map_of_scaled_image_closed_form(s):
    g = torch.Generator().manual_seed(11)
    a = torch.rand((2, 3, 19, 29), generator=g, dtype=torch.float64)
    ssim_map, cs_map, var_a = OE._ssim_maps(a, s * a)
    assert cs_map.shape == (2, 3, 9, 19) and var_a.shape == cs_map.shape
    assert float(var_a.min()) > 1e-2                 # noise: the variance term dominates c2
    want = (2 * s * var_a + C2) / ((1 + s * s) * var_a + C2)
    assert float((cs_map - want).abs().max()) < 1e-9
    # the windowed variance itself, against a direct evaluation of one window
    w = OE._gaussian().flatten()
    w2 = torch.outer(w, w)
    patch = a[1, 2, 3:14, 7:18]
    mu = float((w2 * patch).sum())
    assert float(var_a[1, 2, 3, 7]) == pytest.approx(float((w2 * patch * patch).sum()) - mu * mu, abs=1e-12)
    # per image: the mean of the maps over channels and windows
    sim, cs = OE._ssim_and_cs(a, s * a)
    assert float((cs - cs_map.reshape(2, -1).mean(-1)).abs().max()) < 1e-15
    assert float((sim - ssim_map.reshape(2, -1).mean(-1)).abs().max()) < 1e-15


def test_ms_ssim_relu_clamp_and_dtype():
    g = torch.Generator().manual_seed(13)
    a = torch.rand((2, 3, 177, 203), generator=g, dtype=torch.float64)
    _, cs = OE._ssim_and_cs(a, 1 - a)
    assert float(cs.max()) < -0.9                    # anti-correlated: cs = (c2 - 2 var) / (c2 + 2 var)
    assert OE.ms_ssim(a, 1 - a) == 0.0
    b = (1 - a).clone()
    b[1] = a[1]
    assert OE.ms_ssim(a, b) == pytest.approx(0.5, abs=1e-12)
    # fp32 inputs are pooled in float64 too: the value is that of the same numbers passed as doubles
    a32 = a.float()
    b32 = (a32 + 0.15 * torch.randn(a32.shape, generator=g)).clamp(0, 1)
    assert OE.ms_ssim(a32, b32) == OE.ms_ssim(a32.double(), b32.double())
    assert OE.ssim(a32, b32) == OE.ssim(a32.double(), b32.double())
    # dtype=float32 runs the whole formula in fp32: close to, but not the same as, the float64 value
    lo = OE.ms_ssim(a32, b32, dtype=torch.float32)
    assert lo != OE.ms_ssim(a32, b32) and abs(lo - OE.ms_ssim(a32, b32)) < 1e-5


def test_host_side_argument_rules():
    """checks the device path makes before any launch: MS-SSIM's size rule on both sides (torchmetrics:
    side // 16 > 10), and an Adam group of empty parameters being a no-op"""
    from floodgan import ops
    from floodgan.evaluate import ImageMetrics
    im = ImageMetrics("cpu")
    for h, w in ((191, 161), (161, 191), (160, 160), (31, 400), (400, 31)):
        x = torch.zeros(1, 3, h, w)
        with pytest.raises(ValueError):
            im.ms_ssim(x, x)
    e = torch.empty(0)
    assert ops.adam_step([(e, e, e, e)], 2e-4, 0.5, 0.999, 1e-8, 1) is None
