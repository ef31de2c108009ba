"""Evaluation inference: the reference's Model.calculate_metrics
(models/model.py:363-422) and ModelsGroup.compare_metrics (models/group.py:114-221) on the device.

Per batch of the loader: the generator's forward (torch.manual_seed(47) first, as the reference), the
[0, 1] images clamp((x + 1) * 0.5, 0, 1) of output and target, PSNR / SSIM / MS-SSIM of the pair
(torchmetrics 1.2.0 semantics, requirements.txt:7: data_range=(0, 1), per call = per batch, then
averaged over batches), and the segmentation U-Net's flood masks of both images accumulated into
confusion counts; at the end MSE / accuracy / F1 / precision / recall of the flood and no-flood masks
over every pixel seen (the reference concatenates the flattened masks, which is the same counts).

LPIPS (torchmetrics' LearnedPerceptualImagePatchSimilarity with its defaults: net_type="alex",
reduction="mean", normalize=False, models/model.py:404-406) needs pretrained AlexNet + "lin" weights that
this repository cannot ship: without them it is reported as NaN.  Given a weights file (lpips_weights=, see
load_lpips_weights for the accepted layouts) the LPIPS class computes it on the device: the scaling layer,
AlexNet's stem conv and the pools and the per-tap distance in their own kernels (csrc/lpips.hip), the other
four convs on the conv engine.  The formula implemented, on the [0, 1] images as they are (no 2x - 1 rescale):
  1. x' = (x - shift) / scale per RGB channel, shift (-0.030, -0.088, -0.188), scale (0.458, 0.448, 0.450);
  2. torchvision AlexNet `features` with zero padding applied after the scaling, five taps each after a ReLU:
     Conv(3,64,11,s4,p2) | MaxPool(3,s2) Conv(64,192,5,p2) | MaxPool(3,s2) Conv(192,384,3,p1) |
     Conv(384,256,3,p1) | Conv(256,256,3,p1);
  3. per tap k, n(f) = sqrt(1e-8 + sum_c f_c^2), d_k[i] = mean_{y,x} sum_c w_k[c] (f0_c / n(f0) - f1_c / n(f1))^2;
  4. LPIPS[i] = sum_k d_k[i]; one call = one batch = the mean over i, then averaged over batches.

torchmetrics itself is not installed here (nor is lpips, nor any pretrained weights), so the metric formulas
follow its published 1.2.0 algorithm and their parity is unpinned (the oracle restates the same algorithm:
oracle/evaluation.py; for LPIPS tests/lpips_oracle.py)."""
import math
import os
import time

import numpy as np
import torch

from . import _lib as L
from . import ops
from . import plans as PL
from .segmentation import SegmentationModel, unit_image

MS_SSIM_BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
K1, K2 = 0.01, 0.03
DATA_RANGE = 1.0
METRIC_NAMES = ["PSNR", "SSIM", "MS-SSIM", "LPIPS", "MSE", "Accuracy", "F1_Flood", "Precision_Flood", "Recall_Flood",
                "F1_No_Flood", "Precision_No_Flood", "Recall_No_Flood"]


def gaussian11(sigma=1.5, size=11):
    """torchmetrics _gaussian in float32: exp(-(d / sigma)^2 / 2) over d = -5..5, normalised"""
    d = torch.arange((1 - size) / 2, (1 + size) / 2, 1, dtype=torch.float32)
    g = torch.exp(-torch.pow(d / sigma, 2) / 2)
    return g / g.sum()


class ImageMetrics:
    """Device PSNR / SSIM / MS-SSIM of [N, C, H, W] images already in [0, 1] (contiguous NCHW)."""

    def __init__(self, device="cuda", lpips=None):
        self.device = torch.device(device)
        self._lpips = _as_lpips(lpips, device)
        self.g = gaussian11().to(self.device)
        self.betas = torch.tensor(MS_SSIM_BETAS, dtype=torch.float64, device=self.device)
        self.c1, self.c2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2

    def psnr(self, a, b):
        """10 log10(range^2 / mean squared error over the whole batch) -- one torchmetrics update+compute"""
        out = torch.empty(1, dtype=torch.float64, device=self.device)
        work = torch.empty(int(L.load().fg_sq_err_workspace_doubles()), dtype=torch.float64, device=self.device)
        L.check(L.load().fg_sq_err_sum(L.ptr(a), L.ptr(b), a.numel(), L.ptr(out), L.ptr(work), L.stream_handle()),
                "sq_err_sum")
        mse = float(out) / a.numel()
        return 10.0 * math.log10(DATA_RANGE ** 2 / mse) if mse > 0 else float("inf")

    def _ssim_cs(self, a, b, want_cs=False):
        N, C, H, W = a.shape
        lib = L.load()
        ssim = torch.empty(N, dtype=torch.float64, device=self.device)
        cs = torch.empty(N, dtype=torch.float64, device=self.device) if want_cs else None
        work = torch.empty(int(lib.fg_ssim_workspace_doubles(N, C, H, W)), dtype=torch.float64, device=self.device)
        L.check(lib.fg_ssim(L.ptr(a), L.ptr(b), N, C, H, W, L.ptr(self.g), ops.C.c_float(self.c1),
                            ops.C.c_float(self.c2), L.ptr(ssim), L.ptr(cs), L.ptr(work), L.stream_handle()), "ssim")
        return ssim, cs

    def ssim(self, a, b):
        """mean over the batch of the per-image SSIM"""
        return float(self._ssim_cs(a, b)[0].mean())

    def ms_ssim(self, a, b):
        """torchmetrics MultiScaleStructuralSimilarityIndexMeasure (normalize="relu"): five scales, the
        contrast sensitivity of the first four and the SSIM of the last, F.avg_pool2d(2) in between"""
        N, C, H, W = a.shape
        S = len(MS_SSIM_BETAS)
        if H < 2 ** S or W < 2 ** S or H // (S - 1) ** 2 <= 10 or W // (S - 1) ** 2 <= 10:
            raise ValueError(f"MS-SSIM needs images larger than {(S - 1) ** 2 * 10}px (got {H}x{W})")
        cs_all = torch.empty(S - 1, N, dtype=torch.float64, device=self.device)
        lib = L.load()
        for s in range(S):
            ssim, cs = self._ssim_cs(a, b, want_cs=True)
            if s < S - 1:
                cs_all[s] = cs
                h2, w2 = a.shape[2] // 2, a.shape[3] // 2
                pa = torch.empty(N, C, h2, w2, dtype=torch.float32, device=self.device)
                pb = torch.empty_like(pa)
                for src, dst in ((a, pa), (b, pb)):
                    L.check(lib.fg_avg_pool2(L.ptr(src), N * C, src.shape[2], src.shape[3], L.ptr(dst),
                                             L.stream_handle()), "avg_pool2")
                a, b = pa, pb
        out = torch.empty(N, dtype=torch.float64, device=self.device)
        L.check(lib.fg_msssim_combine(N, S, L.ptr(cs_all), L.ptr(ssim), L.ptr(self.betas), L.ptr(out),
                                      L.stream_handle()), "msssim_combine")
        return float(out.mean())

    def lpips(self, a, b):
        """batch-mean LPIPS (needs ImageMetrics(lpips=weights path / dict / LPIPS object))"""
        if self._lpips is None:
            raise RuntimeError("ImageMetrics.lpips needs LPIPS weights: construct ImageMetrics(lpips=...)")
        return self._lpips(a, b)


# ------------------------------------------------------------------------------------------ LPIPS

LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
# AlexNet features: (index in torchvision's Sequential, lpips slice, out, in, kernel, stride, padding)
ALEX_CONVS = ((0, 1, 64, 3, 11, 4, 2), (3, 2, 192, 64, 5, 1, 2), (6, 3, 384, 192, 3, 1, 1), (8, 4, 256, 384, 3, 1, 1),
              (10, 5, 256, 256, 3, 1, 1))
LPIPS_MIN_SIZE = 31          # the second pool needs a 3 x 3 input: 31 -> 7 -> 3 -> 1


def lpips_weight_shapes():
    """{our fixed name: shape} of the dict load_lpips_weights returns: conv{1..5}.weight / .bias (AlexNet
    features 0, 3, 6, 8, 10) and lin{0..4}.weight (the taps' 1x1 weights, flattened to [C])"""
    out = {}
    for i, (_, _, o, c, k, _, _) in enumerate(ALEX_CONVS):
        out[f"conv{i + 1}.weight"] = (o, c, k, k)
        out[f"conv{i + 1}.bias"] = (o,)
        out[f"lin{i}.weight"] = (o,)
    return out


def load_lpips_weights(path_or_dict):
    """LPIPS (alex) weights as a plain dict of fp32 CPU tensors under the names of lpips_weight_shapes(), from a
    file (torch.load(..., map_location="cpu", weights_only=True)) or a state dict in one of these layouts:
      * lpips / torchmetrics: net.slice1.0 / net.slice2.3 / net.slice3.6 / net.slice4.8 / net.slice5.10
        .{weight,bias}, lin{0..4}.model.1.weight [1, C, 1, 1]; optionally scaling_layer.shift / .scale (must equal
        the constants to 1e-6) and the lins.{k}.model.1.weight aliases a module's state_dict() repeats (must equal
        lin{k}); optionally one extra leading "net." on every key (a metric's state_dict());
      * parts: torchvision AlexNet's features.{0,3,6,8,10}.{weight,bias} merged with the five lin{k}.model.1.weight;
      * the returned dict itself.
    Every shape is checked; a missing key, an unexpected key or a wrong shape raises ValueError naming the key."""
    sd = path_or_dict
    if isinstance(sd, (str, os.PathLike)):
        sd = torch.load(sd, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict) or not sd:
        raise ValueError(f"LPIPS weights: expected a state dict (got {type(sd).__name__})")
    sd = dict(sd)
    shapes = lpips_weight_shapes()
    # a metric's state_dict(): every key, the lin keys too, carries one more "net."
    if all(k.startswith("net.") for k in sd) and any(k.startswith(("net.net.", "net.lin", "net.features."))
                                                     for k in sd):
        sd = {k[4:]: v for k, v in sd.items()}
    if any(k.startswith("net.slice") for k in sd):
        names = {f"net.slice{sl}.{idx}.{p}": f"conv{i + 1}.{p}" for i, (idx, sl, *_) in enumerate(ALEX_CONVS)
                 for p in ("weight", "bias")}
    elif any(k.startswith("features.") for k in sd):
        names = {f"features.{idx}.{p}": f"conv{i + 1}.{p}" for i, (idx, *_) in enumerate(ALEX_CONVS)
                 for p in ("weight", "bias")}
    else:
        names = {k: k for k in shapes if k.startswith("conv")}
    own = not any(k.startswith(("net.slice", "features.")) for k in sd)
    for k in range(5):
        names[f"lin{k}.weight" if own else f"lin{k}.model.1.weight"] = f"lin{k}.weight"
    out = {}
    for src, dst in names.items():
        if src not in sd:
            raise ValueError(f"LPIPS weights: missing key {src!r}")
        want = shapes[dst] if (own or not dst.startswith("lin")) else (1, shapes[dst][0], 1, 1)
        t = sd.pop(src)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
            raise ValueError(f"LPIPS weights: key {src!r} has shape {tuple(getattr(t, 'shape', ()))}, expected {want}")
        out[dst] = t.detach().to(torch.float32).reshape(shapes[dst]).contiguous().clone()
    for src, const in (("scaling_layer.shift", LPIPS_SHIFT), ("scaling_layer.scale", LPIPS_SCALE)):
        if src in sd:
            t = sd.pop(src)
            if t.numel() != 3 or float((t.detach().double().flatten() - torch.tensor(const, dtype=torch.float64))
                                       .abs().max()) > 1e-6:
                raise ValueError(f"LPIPS weights: key {src!r} differs from the scaling layer's constants {const}")
    for k in range(5):
        src = f"lins.{k}.model.1.weight"
        if src in sd:
            t = sd.pop(src)
            if tuple(t.shape) != (1, shapes[f"lin{k}.weight"][0], 1, 1) or not torch.equal(
                    t.detach().to(torch.float32).flatten(), out[f"lin{k}.weight"]):
                raise ValueError(f"LPIPS weights: key {src!r} differs from 'lin{k}.model.1.weight'")
    if sd:
        raise ValueError(f"LPIPS weights: unexpected key {sorted(sd)[0]!r}")
    return out


class LPIPS:
    """torchmetrics LearnedPerceptualImagePatchSimilarity() (alex, mean, normalize=False) on the device, formula as
    in the module docstring (parity unpinned).  weights: a path or a dict (load_lpips_weights).  The conv weights are
    packed once per object (and per conv math), the activation buffers cached per input shape."""

    def __init__(self, weights, device="cuda"):
        self.device = torch.device(device)
        W = {k: v.to(self.device) for k, v in load_lpips_weights(weights).items()}
        self.stem_w = W["conv1.weight"].permute(1, 2, 3, 0).contiguous()       # [c][r][s][64]
        self.conv_w = [W[f"conv{i}.weight"] for i in range(2, 6)]
        self.bias = [W[f"conv{i}.bias"] for i in range(1, 6)]
        self.lin = [W[f"lin{k}.weight"] for k in range(5)]
        self._packs, self._bufs = {}, {}

    def _packed(self, i, c_alloc):
        """(packed weight, weight map) of conv i + 2 in the current conv math"""
        key = (L.get_conv_math(), i)
        if key not in self._packs:
            m = PL.wmap_conv_fwd(self.conv_w[i].shape, c_alloc)
            self._packs[key] = (ops.pack_weight(self.conv_w[i], m), m)
        return self._packs[key]

    def _buffers(self, n, h, w):
        key = (n, h, w)
        if key not in self._bufs:
            dev = self.device
            h0, w0 = PL.out_size(h, 11, 4, 2), PL.out_size(w, 11, 4, 2)
            h1, w1 = PL.out_size(h0, 3, 2, 0), PL.out_size(w0, 3, 2, 0)
            h2, w2 = PL.out_size(h1, 3, 2, 0), PL.out_size(w1, 3, 2, 0)
            # a padded buffer's border is zeroed here once: the kernels write interiors only
            self._bufs[key] = dict(
                t0=PL.Buf.empty(n, h0, w0, 64, 0, dev), p1=PL.Buf.zeros(n, h1, w1, 64, 2, dev),
                t1=PL.Buf.empty(n, h1, w1, 192, 0, dev), p2=PL.Buf.zeros(n, h2, w2, 192, 1, dev),
                t2=PL.Buf.zeros(n, h2, w2, 384, 1, dev), t3=PL.Buf.zeros(n, h2, w2, 256, 1, dev),
                t4=PL.Buf.empty(n, h2, w2, 256, 0, dev), out=torch.empty(n // 2, dtype=torch.float64, device=dev))
        return self._bufs[key]

    def _conv(self, i, X, Y):
        k, pad = ALEX_CONVS[i + 1][4], ALEX_CONVS[i + 1][6]
        wp, m = self._packed(i, X.c)
        ops.conv([PL.conv_problem(X, pad, k, 1, wp, m, Y, bias=self.bias[i + 1], act=L.FG_ACT_RELU)])

    def per_image(self, a, b):
        """[N] fp64 LPIPS of each image pair of two [N, 3, H, W] images in [0, 1]"""
        if a.dim() != 4 or a.shape[1] != 3 or a.shape != b.shape:
            raise ValueError(f"LPIPS takes two [N, 3, H, W] images of equal shape (got {tuple(a.shape)} and "
                             f"{tuple(b.shape)})")
        N, _, H, W = a.shape
        if H < LPIPS_MIN_SIZE or W < LPIPS_MIN_SIZE:
            raise ValueError(f"LPIPS (alex) needs images of at least {LPIPS_MIN_SIZE}px (got {H}x{W})")
        B = self._buffers(2 * N, H, W)
        for img0, x in ((0, a), (N, b)):                       # output and target as one 2N batch
            ops.lpips_stem(x, self.stem_w, self.bias[0], B["t0"], img0)
        ops.maxpool3s2(B["t0"], B["p1"])
        self._conv(0, B["p1"], B["t1"])
        ops.maxpool3s2(B["t1"], B["p2"])
        self._conv(1, B["p2"], B["t2"])
        self._conv(2, B["t2"], B["t3"])
        self._conv(3, B["t3"], B["t4"])
        for k in range(5):
            f0, f1 = ops.half_views(B[f"t{k}"])
            ops.lpips_layer(f0, f1, B[f"t{k}"].c, self.lin[k], B["out"], accumulate=k > 0)
        return B["out"].clone()

    def __call__(self, a, b):
        """the batch mean (reduction="mean"): one torchmetrics update + compute"""
        return float(self.per_image(a, b).mean())


def _as_lpips(lpips_weights, device):
    """None, an LPIPS object, or weights (path / dict) -> None or an LPIPS object"""
    if lpips_weights is None or isinstance(lpips_weights, LPIPS):
        return lpips_weights
    return LPIPS(lpips_weights, device)


class MaskConfusion:
    """tp / fp / tn / fn of the flood masks over every pixel seen, and the torchmetrics binary metrics
    (zero_division -> 0) of the flood and the inverted no-flood masks"""

    def __init__(self, device="cuda"):
        self.counts = torch.zeros(4, dtype=torch.int64, device=device)

    def update(self, pred_logits, true_logits):
        L.check(L.load().fg_mask_confusion(ops.view(pred_logits), ops.view(true_logits), L.ptr(self.counts),
                                           L.stream_handle()), "mask_confusion")

    def compute(self):
        tp, fp, tn, fn = (int(v) for v in self.counts.cpu())
        n = tp + fp + tn + fn

        def div(a, b):
            return a / b if b else 0.0

        out = {"MSE": div(fp + fn, n), "Accuracy": div(tp + tn, n),
               "F1_Flood": div(2 * tp, 2 * tp + fp + fn), "Precision_Flood": div(tp, tp + fp),
               "Recall_Flood": div(tp, tp + fn)}
        # the no-flood masks are 1 - mask: tp <-> tn, fp <-> fn
        out.update({"F1_No_Flood": div(2 * tn, 2 * tn + fn + fp), "Precision_No_Flood": div(tn, tn + fn),
                    "Recall_No_Flood": div(tn, tn + fp)})
        return out


def extract_input_topography(x, topography):
    """models/utils.py:69-79 on a 9-channel input; inputs the loader already narrowed pass through"""
    from .data import TOPOGRAPHY_SOURCE_CHANNELS
    key = None if topography in (None, "none") else topography
    chans = TOPOGRAPHY_SOURCE_CHANNELS[key]
    if x.shape[1] == len(chans):
        return x
    if x.shape[1] != 9:
        raise ValueError(f"input with {x.shape[1]} channels for topography {topography!r}")
    return x[:, chans]


def score_batch(generator, input_stack, ground_truth, seg, im, confs, sync=True, *, with_lpips=False):
    """One batch of models/model.py:388-410 (the segmentation U-Net sees the output, then the target, as
    there): returns (PSNR, SSIM, MS-SSIM, inference seconds); the masks go into every MaskConfusion of
    confs.  with_lpips=True (im built with lpips=): returns (PSNR, SSIM, MS-SSIM, inference seconds, LPIPS)."""
    start = time.time()
    torch.manual_seed(47)
    with torch.no_grad():
        out = generator(input_stack)
    if sync:
        torch.cuda.synchronize()
    t = time.time() - start
    gt, gt_buf = unit_image(ground_truth, buf=True)
    go, go_buf = unit_image(out, buf=True)
    pred_logits = seg.logits_from_buf(go_buf)
    true_logits = seg.logits_from_buf(gt_buf)
    for conf in confs:
        conf.update(pred_logits, true_logits)
    vals = (im.psnr(go, gt), im.ssim(go, gt), im.ms_ssim(go, gt), t)
    return vals + (im.lpips(go, gt),) if with_lpips else vals


_BATCH_KEYS = ("PSNR", "SSIM", "MS-SSIM", "Inference", "LPIPS")


def calculate_metrics(generator, loader, seg_model, topography="all", device="cuda", lpips_weights=None):
    """The device counterpart of Model.calculate_metrics: {metric: value} averaged as the reference
    does (image metrics over batches, mask metrics over all pixels).  lpips_weights (a path, a dict or an
    LPIPS object): LPIPS is the mean of the per-batch values; None: NaN."""
    im, conf = ImageMetrics(device, lpips=lpips_weights), MaskConfusion(device)
    with_lpips = lpips_weights is not None
    per = {k: [] for k in _BATCH_KEYS}
    for input_stack, ground_truth, _ in loader:
        x = extract_input_topography(input_stack, topography).to(device)
        y = ground_truth.to(device)
        for k, v in zip(_BATCH_KEYS, score_batch(generator, x, y, seg_model, im, [conf], with_lpips=with_lpips)):
            per[k].append(v)
    res = {k: float(np.mean(v)) for k, v in per.items() if k not in ("Inference", "LPIPS")}
    res["LPIPS"] = float(np.mean(per["LPIPS"])) if with_lpips else float("nan")
    res.update(conf.compute())
    res["Inference"] = float(np.mean(per["Inference"]))
    return {k: res[k] for k in METRIC_NAMES + ["Inference"]}


def compare_metrics(generators, loader, seg_model, compare="model", device="cuda", lpips_weights=None):
    """ModelsGroup.compare_metrics (models/group.py:114-221): {generator name: {metric: value}} plus the
    per-disaster metrics {generator name: {disaster: {metric: value}}} -- the mask metrics over that
    disaster's pixels and the batch means of PSNR / SSIM / MS-SSIM / LPIPS (NaN without lpips_weights: a path, a
    dict or an LPIPS object) over its batches, as the reference's grouped table (group.py:211-221).
    compare="topography": the
    generators are keyed by topography ("All", "DEM", "Flow accumulation", "Distance to rivers", "Map",
    "None") and see the matching channels of one 9-channel input (models/group.py:83-94)."""
    topo_keys = _TOPOGRAPHY_KEYS
    im = ImageMetrics(device, lpips=lpips_weights)
    with_lpips = lpips_weights is not None
    conf = {g: MaskConfusion(device) for g in generators}
    grouped = {}
    per = {g: {k: [] for k in _BATCH_KEYS} for g in generators}
    disasters = []
    for input_stack, ground_truth, names in loader:
        x = input_stack.to(device)
        y = ground_truth.to(device)
        disaster = names[0].split("_")[0]
        disasters.append(disaster)
        for g, gen in generators.items():
            xi = extract_input_topography(x, topo_keys[g]) if compare == "topography" else x
            key = (g, disaster)
            if key not in grouped:
                grouped[key] = MaskConfusion(device)
            im_vals = score_batch(gen, xi, y, seg_model, im, [conf[g], grouped[key]], with_lpips=with_lpips)
            for k, v in zip(_BATCH_KEYS, im_vals):
                per[g][k].append(v)
    out = {}
    for g in generators:
        res = {k: float(np.mean(v)) for k, v in per[g].items() if k not in ("Inference", "LPIPS")}
        res["LPIPS"] = float(np.mean(per[g]["LPIPS"])) if with_lpips else float("nan")
        res.update(conf[g].compute())
        inf = per[g]["Inference"][5:] if g == next(iter(generators)) else per[g]["Inference"]   # group.py:198-200
        res["Inference"] = float(np.mean(inf)) if inf else float("nan")
        out[g] = {k: res[k] for k in METRIC_NAMES + ["Inference"]}
    by_disaster = {}
    for (g, d), c in grouped.items():
        vals = {k: float(np.mean([v for v, dd in zip(per[g][k], disasters) if dd == d]))
                for k in ("PSNR", "SSIM", "MS-SSIM") + (("LPIPS",) if with_lpips else ())}
        vals.setdefault("LPIPS", float("nan"))
        vals.update(c.compute())
        by_disaster.setdefault(g, {})[d] = vals
    return out, by_disaster


_TOPOGRAPHY_KEYS = {"All": "all", "DEM": "dem", "Flow accumulation": "flow", "Distance to rivers": "river", "Map": "map",
                    "None": None}


def compare_output_images(generators, image_names, *, compare="model", data_path, dataset_dem="best", topography="all",
                          resize=256, crop=None, crop_index=0, csv_path="metadata/dataset_split.csv", out_path,
                          device="cuda"):
    """ModelsGroup.compare_output_images (models/group.py:223-280): one sheet (floodgan.render.save_sheet) with a
    row per image name -- a trailing _k is its crop index, else crop_index -- and the columns input | ground truth |
    one per generator of `generators` ({name: module}), each called under torch.manual_seed(47).
    compare="topography": the tiles are loaded with all nine channels and every generator, keyed by topography as in
    compare_metrics, sees its channels (extract_input_topography).  Written to out_path (the reference's
    create_path("image", info=...)); returns the sheet's panels dict."""
    from .data import load_image_pair
    from .render import save_sheet
    xs, ys, names = [], [], []
    outs = {g: [] for g in generators}
    for image_name in image_names:
        final_crop_index = crop_index
        if len(image_name) >= 2 and image_name[-2] == "_":                      # models/group.py:237-241
            final_crop_index, image_name = int(image_name[-1]), image_name[:-2]
        x, y, name = load_image_pair(image_name, data_path, dataset_dem, "all" if compare == "topography" else
                                     topography, resize, crop, final_crop_index, csv_path=csv_path, device=device)
        for g, gen in generators.items():
            xi = extract_input_topography(x, _TOPOGRAPHY_KEYS[g]) if compare == "topography" else x
            torch.manual_seed(47)
            with torch.no_grad():
                outs[g].append(gen(xi.detach().clone()))
        xs.append(x)
        ys.append(y)
        names.append(name)
    cols = [("Input", "rgb", xs), ("Ground truth", "rgb", ys)] + [(str(g), "rgb", outs[g]) for g in generators]
    return save_sheet(out_path, cols, names)


def segmentation_model(seg_model_path=None, device="cuda"):
    return SegmentationModel(pretrained_model_path=seg_model_path, device=device).model
