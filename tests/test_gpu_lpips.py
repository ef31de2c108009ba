"""LPIPS on the HIP path (csrc/lpips.hip, floodgan.evaluate.LPIPS) against the fp64 restatement in
tests/lpips_oracle.py (torchmetrics parity unpinned: no library, no pretrained weights): each new kernel on its
own, the whole metric, and its wiring into calculate_metrics / compare_metrics.

Kernel outputs start NaN-filled: an element that must be written comes out finite, and a border the kernel must leave
alone keeps its NaN.  The bounds come from tests/lpips_oracle.py (fp32 torch vs fp64 on the CPU), never from the HIP
path.  Measured on the MI355X (default f16x3 conv math):
  stem, max |error| / max |reference|: 6.6e-07 (35x47), 7.2e-07 (64x64) against KTOL = 1e-5;
  layer distance, worst relative error 1.6e-07 (192 channels, 1x2) against the bound min(4 x 1.55e-07, 1e-6) =
  6.2e-07;
  end to end, worst per-image |error| 1.4e-08 (2 x 35x47, bounds 9.9e-08 / 9.3e-08) and 5.2e-09 (1 x 67x95, bound
  1.1e-07), the fp32 torch oracle's worst relative error being 3.9e-07."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_oracle as LO
from test_gpu_parity import DEV, KTOL

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from floodgan import _lib as L
    L.load()
    L.check(L.load().fg_device_ok(), "device_ok")


def _nan_buf(n, h, w, c, pad):
    from floodgan.plans import Buf
    return Buf(torch.full((n * (h + 2 * pad) * (w + 2 * pad) * c,), NAN, dtype=torch.float32, device=DEV), n, h, w, c,
               pad)


def _buf_of(x_nchw, pad):
    """NHWC Buf holding x in its interior; the border is NaN (the kernels under test must not read it)"""
    n, c, h, w = x_nchw.shape
    B = _nan_buf(n, h, w, c, pad)
    B.interior().copy_(x_nchw.float().permute(0, 2, 3, 1).to(DEV))
    return B


def _interior_nchw(B):
    return B.interior().permute(0, 3, 1, 2).double().cpu()


def _border_is_nan(B):
    full = B.nhwc().clone()
    p = B.pad
    if p == 0:
        return True
    full[:, p:p + B.h, p:p + B.w, :] = NAN
    return bool(torch.isnan(full).all())


# ------------------------------------------------------------------ stem

@pytest.mark.parametrize("n,h,w", [(2, 35, 47), (1, 64, 64)])
def test_stem_vs_fp64(n, h, w, report):
    """scaling layer + zero pad + 11x11 stride-4 conv + bias + ReLU; the image's border pixels are non-zero (a
    uniform random image), so padding before the scaling would show: the CPU sensitivity test measures by how much"""
    from floodgan import ops
    from floodgan.evaluate import load_lpips_weights
    g = torch.Generator().manual_seed(h * w)
    x = torch.rand((n, 3, h, w), generator=g)
    assert float(x[:, :, 0].min()) > 0 and float(x[:, :, :, -1].min()) > 0
    sd = LO.seeded_weights()
    ref = LO.stem(x, sd)
    wrong = LO.stem(x, sd, pad_after_scaling=False)
    W = load_lpips_weights(sd)
    wt = W["conv1.weight"].permute(1, 2, 3, 0).contiguous().to(DEV)
    ho, wo = ref.shape[2:]
    # the batch lands at image 1 of a wider buffer: images 0 and n + 1 must stay untouched
    Y = _nan_buf(n + 2, ho, wo, 64, 0)
    ops.lpips_stem(x.to(DEV), wt, W["conv1.bias"].to(DEV), Y, img0=1)
    got = _interior_nchw(Y)
    assert torch.isnan(got[0]).all() and torch.isnan(got[n + 1]).all()
    got = got[1:n + 1]
    assert torch.isfinite(got).all()
    err = float((got - ref).abs().max() / ref.abs().max())
    seen = float((wrong - ref).abs().max() / ref.abs().max())
    print(f"lpips stem {n}x{h}x{w}: max error / max |ref| = {err:.3e} (padding before the scaling would be {seen:.1e})")
    report("lpips_stem", n=n, h=h, w=w, err=err)
    assert seen > 100 * KTOL
    assert err < KTOL
    assert bool(((got == 0) == (ref <= 0))[ref.abs() > 1e-4].all())           # the ReLU


def test_stem_takes_strided_input():
    from floodgan import ops
    from floodgan.evaluate import load_lpips_weights
    g = torch.Generator().manual_seed(3)
    x = torch.rand((1, 35, 47, 3), generator=g).permute(0, 3, 1, 2)            # channels-last strides
    sd = LO.seeded_weights()
    ref = LO.stem(x, sd)
    W = load_lpips_weights(sd)
    Y = _nan_buf(1, 8, 11, 64, 0)
    ops.lpips_stem(x.to(DEV), W["conv1.weight"].permute(1, 2, 3, 0).contiguous().to(DEV), W["conv1.bias"].to(DEV), Y)
    assert float((_interior_nchw(Y) - ref).abs().max() / ref.abs().max()) < KTOL


# ------------------------------------------------------------------ pool

@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("c", [64, 192])
@pytest.mark.parametrize("h,w", [(8, 11), (15, 15)])
def test_maxpool3s2_exact(h, w, c, pad):
    from floodgan import ops
    g = torch.Generator().manual_seed(h * 1000 + c + pad)
    x = F.relu(torch.randn((2, c, h, w), generator=g))
    ref = F.max_pool2d(x.double(), 3, 2)
    assert tuple(ref.shape[2:]) == {(8, 11): (3, 5), (15, 15): (7, 7)}[h, w]
    src = _buf_of(x, 1)                                     # a NaN border around the source: it is never read
    dst = _nan_buf(2, ref.shape[2], ref.shape[3], c, pad)
    ops.maxpool3s2(src, dst)
    assert torch.equal(_interior_nchw(dst), ref)
    assert _border_is_nan(dst)


# ------------------------------------------------------------------ layer distance

@pytest.mark.parametrize("c,h,w", LO.LAYER_CASES)
def test_layer_distance_vs_fp64(c, h, w, report):
    """one tap's d_k: pixels whose vectors are entirely zero in one / both inputs, a nearly dead pixel, an identical
    pair (exactly 0); the two inputs as the halves of one 2N batch and as two buffers with different borders"""
    from floodgan import ops
    f0, f1, lw = LO.layer_inputs(c, h, w)
    ref = LO.layer_reference(c, h, w)
    bound = LO.layer_bound()
    lwd = lw.to(DEV)
    both = _buf_of(torch.cat([f0, f1]), 1)
    outs = []
    for _ in range(2):
        out = torch.full((2,), NAN, dtype=torch.float64, device=DEV)
        ops.lpips_layer(*ops.half_views(both), c, lwd, out)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])                                        # bit-identical runs
    out2 = torch.full((2,), NAN, dtype=torch.float64, device=DEV)
    ops.lpips_layer(_buf_of(f0, 0), _buf_of(f1, 2), c, lwd, out2)
    assert torch.equal(out2.cpu(), outs[0])
    ops.lpips_layer(_buf_of(f0, 0), _buf_of(f1, 2), c, lwd, out2, accumulate=True)
    assert torch.equal(out2.cpu(), outs[0] + outs[0])
    got = outs[0]
    rel = float(abs(got[0] - ref[0]) / ref[0])
    print(f"lpips layer c={c} {h}x{w}: got {got.tolist()} ref {ref.tolist()} relative error {rel:.3e} "
          f"(bound {bound:.3e}; fp32 torch {LO.layer_fp32_error():.3e})")
    report("lpips_layer", c=c, h=h, w=w, rel=rel, bound=bound, fp32_torch=LO.layer_fp32_error())
    assert float(got[1]) == 0.0 and float(ref[1]) == 0.0
    assert rel <= bound


def test_layer_rejects_bad_channels():
    from floodgan import ops
    f = _buf_of(torch.rand(2, 96, 3, 3), 0)
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ops.lpips_layer(*ops.half_views(f), 96, torch.rand(96, device=DEV), out)


# ------------------------------------------------------------------ end to end

@pytest.fixture(scope="module")
def metric():
    from floodgan.evaluate import LPIPS
    return LPIPS(LO.weights(), DEV)


@pytest.mark.parametrize("n,h,w", LO.E2E_CASES)
def test_lpips_end_to_end(n, h, w, metric, report):
    a, b = LO.e2e_inputs(n, h, w)
    ref, e32 = LO.e2e_reference(n, h, w)[0], LO.e2e_fp32_error()
    bound = LO.e2e_bound(n, h, w)
    ad, bd = a.to(DEV), b.to(DEV)
    per = metric.per_image(ad, bd)
    assert per.dtype == torch.float64 and tuple(per.shape) == (n,)
    per = per.cpu()
    errs = (per - ref).abs()
    mean = metric(ad, bd)
    print(f"lpips end to end {n}x{h}x{w}: got {per.tolist()} ref {ref.tolist()} per-image errors {errs.tolist()} "
          f"mean error {abs(mean - float(ref.mean())):.3e}; fp32 torch relative error {e32:.3e} (this case "
          f"{LO.e2e_reference(n, h, w)[1].tolist()}), bounds {bound.tolist()}")
    report("lpips_end_to_end", n=n, h=h, w=w, err=float(errs.max()), rel=float((errs / ref).max()), fp32_torch_rel=e32,
           bound=bound.tolist())
    assert torch.equal(metric.per_image(ad, bd).cpu(), per)                    # cached buffers, same bits
    assert float(metric.per_image(ad, ad).abs().max()) <= float(bound.min())   # the oracle gives exactly 0
    for i in range(n):
        assert float(errs[i]) <= float(bound[i]), (i, float(errs[i]), float(bound[i]))
    assert abs(mean - float(ref.mean())) <= float(bound.max())


def test_lpips_input_validation(metric):
    ok = torch.rand(1, 3, 31, 31, device=DEV)
    assert np.isfinite(metric(ok, ok.flip(3)))
    for bad in (torch.rand(1, 3, 30, 40, device=DEV), torch.rand(1, 3, 40, 30, device=DEV)):
        with pytest.raises(ValueError, match="31"):
            metric(bad, bad)
    with pytest.raises(ValueError):
        metric(torch.rand(1, 4, 40, 40, device=DEV), torch.rand(1, 4, 40, 40, device=DEV))
    with pytest.raises(ValueError):
        metric(torch.rand(1, 3, 40, 40, device=DEV), torch.rand(1, 3, 40, 41, device=DEV))


# ------------------------------------------------------------------ wiring

class _TinyGenerator(torch.nn.Module):
    """a fixed map of the input's first three channels to an image in [-1, 1]"""

    def __init__(self, gain):
        super().__init__()
        self.gain = gain

    def forward(self, x):
        return torch.tanh(self.gain * x[:, :3] + 0.1)


def _loader():
    g = torch.Generator().manual_seed(11)
    R = 176                                                 # the smallest size MS-SSIM takes
    return [(torch.rand((1, 9, R, R), generator=g) * 2 - 1, torch.rand((1, 3, R, R), generator=g) * 2 - 1,
             [f"{name}_0"]) for name in ("hurricane-harvey", "midwest-flooding")]


def _per_batch_lpips(gen, loader, metric):
    from floodgan.segmentation import unit_image
    vals = []
    for x, y, _ in loader:
        with torch.no_grad():
            out = gen(x.to(DEV))
        vals.append(metric(unit_image(out)[0], unit_image(y.to(DEV))[0]))
    return vals


def test_metrics_tables_carry_lpips(metric, tmp_path):
    from floodgan.evaluate import METRIC_NAMES, calculate_metrics, compare_metrics
    from test_gpu_evaluation import _unet
    seg = _unet().to(DEV)
    loader = _loader()
    gens = {"A": _TinyGenerator(0.7).to(DEV), "B": _TinyGenerator(1.3).to(DEV)}
    want = {g: _per_batch_lpips(gen, loader, metric) for g, gen in gens.items()}
    assert all(np.isfinite(v) and v > 0 for vs in want.values() for v in vs)
    path = tmp_path / "alex.pth"
    torch.save(LO.weights(), path)

    base = calculate_metrics(gens["A"], loader, seg, topography="all", device=DEV)
    assert list(base) == METRIC_NAMES + ["Inference"] and np.isnan(base["LPIPS"])
    for given in (metric, LO.weights(), str(path)):                             # an object, a dict, a path
        res = calculate_metrics(gens["A"], loader, seg, topography="all", device=DEV, lpips_weights=given)
        assert list(res) == list(base)
        assert res["LPIPS"] == float(np.mean(want["A"]))
        assert all(res[k] == base[k] for k in base if k not in ("LPIPS", "Inference"))

    table0, by0 = compare_metrics(gens, loader, seg, device=DEV)
    assert all(np.isnan(table0[g]["LPIPS"]) for g in gens)
    assert all(np.isnan(v["LPIPS"]) for g in gens for v in by0[g].values())
    table, by = compare_metrics(gens, loader, seg, device=DEV, lpips_weights=metric)
    for g in gens:
        assert table[g]["LPIPS"] == float(np.mean(want[g]))
        assert list(table[g]) == list(table0[g])
        for (_, _, names), v in zip(loader, want[g]):
            d = by[g][names[0].split("_")[0]]
            assert d["LPIPS"] == v and list(d) == list(by0[g][names[0].split("_")[0]])
    assert table["A"]["LPIPS"] != table["B"]["LPIPS"]


def test_score_batch_keeps_its_arity(metric):
    from floodgan.evaluate import ImageMetrics, MaskConfusion, score_batch
    from test_gpu_evaluation import _unet
    seg = _unet().to(DEV)
    x, y, _ = _loader()[0]
    gen = _TinyGenerator(0.7).to(DEV)
    plain = score_batch(gen, x.to(DEV), y.to(DEV), seg, ImageMetrics(DEV), [MaskConfusion(DEV)])
    assert len(plain) == 4
    im = ImageMetrics(DEV, lpips=metric)
    assert len(score_batch(gen, x.to(DEV), y.to(DEV), seg, im, [MaskConfusion(DEV)])) == 4
    more = score_batch(gen, x.to(DEV), y.to(DEV), seg, im, [MaskConfusion(DEV)], with_lpips=True)
    assert len(more) == 5 and more[:3] == plain[:3] and more[4] == _per_batch_lpips(gen, [(x, y, None)], metric)[0]
    with pytest.raises(RuntimeError, match="LPIPS weights"):
        ImageMetrics(DEV).lpips(x[:, :3].to(DEV), y.to(DEV))
