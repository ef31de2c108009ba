"""Plain-torch restatement of the LPIPS the HIP path implements (floodgan/evaluate.py items 1-4: torchmetrics 1.2.0
LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=False), parity unpinned -- neither torchmetrics nor
lpips nor pretrained weights are available), with seeded weights and the inputs both LPIPS test files share.  Checker
only: nothing here is imported by the package.

Bounds.  The GPU tests hold the HIP path to a multiple of the gap between this oracle run in plain fp32 torch on the
CPU and in fp64 -- never to anything measured on the HIP path:
  * end to end: E = the largest relative |fp32 - fp64| error over every image of every end-to-end case; an image
    with fp64 value v gets 4 E v, a batch mean (whose error cannot exceed its worst image's) 4 E max(v).  One draw
    of a rounding error can land arbitrarily close to zero (3.9e-10 on a value of 0.07 was seen for one image, 0.08
    fp32 ulp), so a single image's own gap is no measure of the fp32-to-fp64 gap; the worst over the inputs is;
  * one tap's distance: E = the largest relative fp32-vs-fp64 error over every image of every layer case; the kernel
    gets min(4 E, 1e-6) relative (a different summation order, never looser than 1e-6)."""
import functools

import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (lpips key stem, out, in, kernel, stride, padding, max-pool before the conv)
CONVS = (("net.slice1.0", 64, 3, 11, 4, 2, False), ("net.slice2.3", 192, 64, 5, 1, 2, True),
         ("net.slice3.6", 384, 192, 3, 1, 1, True), ("net.slice4.8", 256, 384, 3, 1, 1, False),
         ("net.slice5.10", 256, 256, 3, 1, 1, False))
FEATURES = (0, 3, 6, 8, 10)          # the same convs in torchvision AlexNet's `features`
EPS = 1e-8

E2E_CASES = ((2, 35, 47), (1, 67, 95))
LAYER_CASES = tuple((c, h, w) for c in (64, 192, 384) for h, w in ((1, 2), (3, 5), (15, 15)))


@functools.lru_cache(maxsize=None)
def seeded_weights(seed=20240):
    """state dict in the lpips / torchmetrics layout: conv weights N(0, 0.05), biases N(0, 0.1), lin weights
    uniform [0, 1) (real lin weights are non-negative)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, (name, o, c, ks, _, _, _) in enumerate(CONVS):
        sd[f"{name}.weight"] = torch.randn((o, c, ks, ks), generator=g) * 0.05
        sd[f"{name}.bias"] = torch.randn((o,), generator=g) * 0.1
        sd[f"lin{k}.model.1.weight"] = torch.rand((1, o, 1, 1), generator=g)
    return sd


def weights():
    """a fresh copy of the seeded state dict (callers may edit it)"""
    return {k: v.clone() for k, v in seeded_weights().items()}


def parts_layout(sd):
    """the same weights keyed as torchvision AlexNet features + the lin layers"""
    out = {}
    for (name, *_), idx in zip(CONVS, FEATURES):
        for p in ("weight", "bias"):
            out[f"features.{idx}.{p}"] = sd[f"{name}.{p}"]
    out.update({k: v for k, v in sd.items() if k.startswith("lin")})
    return out


def stem(x, sd, dtype=torch.float64, scaling=True, pad_after_scaling=True):
    """tap 0: scaling layer, zero pad 2, Conv(3, 64, 11, s4), ReLU"""
    x = x.to(dtype)
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    name, _, _, _, s, p, _ = CONVS[0]
    w, b = sd[f"{name}.weight"].to(dtype), sd[f"{name}.bias"].to(dtype)
    if not scaling:
        return F.relu(F.conv2d(x, w, b, stride=s, padding=p))
    if pad_after_scaling:
        return F.relu(F.conv2d((x - shift) / scale, w, b, stride=s, padding=p))
    return F.relu(F.conv2d((F.pad(x, (p,) * 4) - shift) / scale, w, b, stride=s))     # the wrong order


def taps(x, sd, dtype=torch.float64, **stem_kw):
    """the five post-ReLU feature maps of one image batch"""
    f = stem(x, sd, dtype, **stem_kw)
    out = [f]
    for name, _, _, _, s, p, pool in CONVS[1:]:
        if pool:
            f = F.max_pool2d(f, 3, 2)
        f = F.relu(F.conv2d(f, sd[f"{name}.weight"].to(dtype), sd[f"{name}.bias"].to(dtype), stride=s, padding=p))
        out.append(f)
    return out


def layer_distance(f0, f1, w, dtype=torch.float64, eps_form="sqrt"):
    """[N] d_k of two [N, C, H, W] feature maps, w: [C] (or [1, C, 1, 1]).  eps_form "sqrt": n = sqrt(1e-8 +
    sum f^2) (implemented); "add": f / (sqrt(sum f^2) + 1e-10), the older lpips form (sensitivity guard only)"""
    f0, f1, w = f0.to(dtype), f1.to(dtype), w.to(dtype).reshape(1, -1, 1, 1)

    def unit(f):
        ss = (f * f).sum(1, keepdim=True)
        return f / torch.sqrt(EPS + ss) if eps_form == "sqrt" else f / (torch.sqrt(ss) + 1e-10)

    d = (unit(f0) - unit(f1)) ** 2
    return (d * w).sum(1, keepdim=True).mean((2, 3)).reshape(-1)


def lpips(a, b, sd, dtype=torch.float64, drop_tap=None, **stem_kw):
    """[N] LPIPS of two [N, 3, H, W] images in [0, 1] (passed as they are: no 2x - 1 rescale)"""
    ta, tb = taps(a, sd, dtype, **stem_kw), taps(b, sd, dtype, **stem_kw)
    total = 0
    for k, (fa, fb) in enumerate(zip(ta, tb)):
        if k != drop_tap:
            total = total + layer_distance(fa, fb, sd[f"lin{k}.model.1.weight"], dtype)
    return total


# ------------------------------------------------------------------ shared inputs (seeded, never modified)

@functools.lru_cache(maxsize=None)
def e2e_inputs(n, h, w):
    """an image pair in [0, 1] like a generator output and its target: b = a perturbed; non-zero border pixels"""
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w)
    a = torch.rand((n, 3, h, w), generator=g)
    b = (a + 0.2 * torch.randn((n, 3, h, w), generator=g)).clamp(0, 1)
    return a, b


@functools.lru_cache(maxsize=None)
def e2e_reference(n, h, w):
    """(fp64 per-image oracle, the fp32 oracle's per-image relative errors) of e2e_inputs(n, h, w)"""
    a, b = e2e_inputs(n, h, w)
    sd = seeded_weights()
    ref = lpips(a, b, sd, torch.float64)
    return ref, (lpips(a, b, sd, torch.float32).double() - ref).abs() / ref


@functools.lru_cache(maxsize=None)
def e2e_fp32_error():
    """E: the largest relative error of the fp32 torch oracle against fp64 over every end-to-end case and image"""
    return max(float(e2e_reference(*case)[1].max()) for case in E2E_CASES)


def e2e_bound(n, h, w):
    """[N] absolute bounds, one per image of the case"""
    return 4.0 * e2e_fp32_error() * e2e_reference(n, h, w)[0]


@functools.lru_cache(maxsize=None)
def layer_inputs(c, h, w):
    """N = 2 feature pairs shaped like post-ReLU taps (about half the entries zero) and the lin weight.  Image 0:
    pixel 0 all-zero in f0 only, the last pixel all-zero in both (the eps path) and -- from 3 x 5 up -- pixel 1 of
    f0 nearly dead (norm ~ 1e-4, where the two eps forms differ most); image 1: f1 == f0 (exactly 0)."""
    g = torch.Generator().manual_seed(100000 * c + 100 * h + w)
    f0 = F.relu(torch.randn((2, c, h, w), generator=g))
    f1 = F.relu(f0 + 0.5 * torch.randn((2, c, h, w), generator=g))
    f0[0, :, 0, 0] = 0
    f0[0, :, -1, -1] = 0
    f1[0, :, -1, -1] = 0
    if h * w > 2:
        f0[0, :, 0, 1] *= 1e-5
    f1[1] = f0[1]
    return f0, f1, torch.rand((c,), generator=g)


@functools.lru_cache(maxsize=None)
def layer_reference(c, h, w):
    f0, f1, lw = layer_inputs(c, h, w)
    return layer_distance(f0, f1, lw, torch.float64)


@functools.lru_cache(maxsize=None)
def layer_fp32_error():
    """E: the largest relative error of the fp32 torch evaluation against fp64 over every layer case and image"""
    worst = 0.0
    for case in LAYER_CASES:
        f0, f1, lw = layer_inputs(*case)
        ref = layer_reference(*case)
        got = layer_distance(f0, f1, lw, torch.float32).double()
        nz = ref != 0
        worst = max(worst, float(((got - ref).abs()[nz] / ref[nz]).max()))
    return worst


def layer_bound():
    return min(4.0 * layer_fp32_error(), 1e-6)
