"""The conv engine (csrc/conv_gemm.hip, conv_f3.hip, conv_wgrad_f3.hip) against torch CPU fp64 at the conv
geometries of the two U-Nets -- the flood-segmentation U-Net's DoubleConvs and ConvTranspose2d(2, 2, 0), Pix2Pix
U-Net-256's 4x4 stride-2 down convs and ConvTranspose2d(4, 2, 1) -- in every conv math, each comparison held to the
single-kernel bound KTOL.  The whole-network tests (test_gpu_pix2pix.py, test_gpu_seg_train.py) reach these layers
only through teacher-forced gradients at 1e-4 and in the default math.

Each case is the smallest shape that still has the edge it is there for: M = 4 and M = N output rows (fewer than one
32-row wave block of a 128..512-row tile), 512 / 1024 output channels (4-8 N tiles), K up to 9216, single-tap
transposed phases (kh = 1, K = C), transposed phases over a 1 x 1 input that is mostly zero border, two problems with
different n_base in one launch, outputs that are channel slices of a wider cat buffer, 3 outputs in a 4-channel
buffer and a 3-in-4-channel input (j_valid < jp).

Outputs start NaN-filled: everything that must be written comes out finite and everything else -- borders, the other
half of a cat buffer, channels >= n_out -- keeps its NaN.  Inputs are poisoned nowhere: their border and padding
channels are read by contract and hold zeros.  The kernel family each launch ran (fg_last_launch) is recorded and
asserted where the dispatch (fg_conv_fwd, fgc::f3_takes, fgc::launch_wgrad_f3) decides it by the case's geometry."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import DEV, KTOL, MATHS, buf_from, conv_math, nchw, nrel  # noqa: F401  (conv_math: fixture)

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from floodgan import _lib as L
    L.load()
    L.check(L.load().fg_device_ok(), "device_ok")


_WORST = {}      # (group, math label) -> (worst nrel, "case:what")


@pytest.fixture(scope="module", autouse=True)
def _worst_per_group(report):
    yield
    for (group, label), (err, where) in sorted(_WORST.items()):
        report("unet_convs_worst", group=group, math=label, nrel=err, where=where)


def _record(report, group, case, label, errs, kernels):
    """log one case's errors and kernel families, then hold every error to KTOL"""
    print(f"unet conv {group} {case} [{label}]: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()), kernels)
    report("unet_convs", group=group, case=case, math=label, kernels=kernels, **errs)
    for what, e in errs.items():
        if e > _WORST.get((group, label), (-1.0, ""))[0]:
            _WORST[group, label] = (e, f"{case}:{what}")
    for what, e in errs.items():
        assert e < KTOL, (group, case, label, what, e)


# ------------------------------------------------------------------ engine variants

@contextlib.contextmanager
def _f16x3(f3_tile=-1):
    """the f16x3 math; f3_tile = -2: the pipelined forward kernel off (the register-staged f16x3 kernel runs)"""
    from floodgan import _lib as L
    prev = L.get_conv_math()
    L.set_conv_math("f16x3")
    try:
        L.set_f3_tile(f3_tile)
        yield
    finally:
        L.set_f3_tile(-1)
        L.set_conv_math(prev)


def _fwd_family(math, pipelined):
    """the fg::launched tag of fg_conv_fwd: the pipelined kernel exists in the f16x3 math only"""
    return {"fp32": "conv_fwd", "bf16x6": "conv_fwd_x6"}.get(math, "conv_fwd_f3" if pipelined else "conv_fwd_x6")


def _wgrad_family(math, pipelined):
    return {"fp32": "conv_wgrad", "bf16x6": "conv_wgrad_x6"}.get(math,
                                                                 "conv_wgrad_f3" if pipelined else "conv_wgrad_x6")


# ------------------------------------------------------------------ fp64 references (computed once, never modified)

def _seed(*key):
    return 7919 + sum((i + 1) * int(v) for i, v in enumerate(key))


@functools.lru_cache(maxsize=None)
def _ref_conv(cin, cout, N, H, W, k, s, p, bias, mag=1.0):
    """torch CPU fp64 Conv2d(cin, cout, k, s, p): operands, output, and autograd's gradients for a random gy"""
    g = torch.Generator().manual_seed(_seed(cin, cout, N, H, W, k, s))
    x = torch.randn((N, cin, H, W), dtype=torch.float64, generator=g) * mag
    w = torch.randn((cout, cin, k, k), dtype=torch.float64, generator=g) * 0.05
    b = torch.randn((cout,), dtype=torch.float64, generator=g) * mag if bias else None
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, b, stride=s, padding=p)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=g) * mag
    gx, gw = torch.autograd.grad(y, (xr, wr), gy)
    return dict(x=x, w=w, b=b, y=y.detach(), gy=gy, gx=gx, gw=gw)


@functools.lru_cache(maxsize=None)
def _ref_convT(cin, cout, N, H, W, k, p, mag=1.0):
    """torch CPU fp64 ConvTranspose2d(cin, cout, k, 2, p) with bias"""
    g = torch.Generator().manual_seed(_seed(cin, cout, N, H, W, k, 2, 1))
    x = torch.randn((N, cin, H, W), dtype=torch.float64, generator=g) * mag
    w = torch.randn((cin, cout, k, k), dtype=torch.float64, generator=g) * 0.05
    b = torch.randn((cout,), dtype=torch.float64, generator=g) * mag
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv_transpose2d(xr, wr, b, stride=2, padding=p)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=g) * mag
    gx, gw = torch.autograd.grad(y, (xr, wr), gy)
    return dict(x=x, w=w, b=b, y=y.detach(), gy=gy, gx=gx, gw=gw)


# ------------------------------------------------------------------ writes and nothing but writes

def _nan_buf(n, h, w, c, pad=0):
    from floodgan.plans import Buf
    return Buf(torch.full((n * (h + 2 * pad) * (w + 2 * pad) * c,), NAN, dtype=torch.float32, device=DEV), n, h, w, c,
               pad)


def _only_wrote(B, c0, n_out):
    """B (NaN-filled before the launch): interior channels [c0, c0 + n_out) are finite, everything else -- the
    border, the other channels -- is still NaN"""
    full = B.nhwc().cpu()
    written = torch.zeros(full.shape, dtype=torch.bool)
    written[:, B.pad:B.pad + B.h, B.pad:B.pad + B.w, c0:c0 + n_out] = True
    assert bool(torch.isfinite(full[written]).all()), "an output element was not written (or is not finite)"
    assert bool(torch.isnan(full[~written]).all()), "a launch wrote outside its output"


def _nan_like(t):
    return torch.full(t.shape, NAN, dtype=torch.float32, device=DEV)


def _dev(t):
    return t.float().to(DEV)


# ------------------------------------------------------------------ DoubleConv: 3x3, stride 1, zero pad 1

# (cin, c_alloc, cout, N, H, W, pipelined forward?, pipelined weight gradient?, pipelined input gradient?)
# pipelined (f16x3, defaults): forward / input gradient -- fgc::f3_takes: more than 32 outputs, jp % 32 == 0,
# j_valid == jp; weight gradient -- fgc::launch_wgrad_f3: n_a >= 64, K >= 256
DC_CASES = [
    (3, 4, 64, 2, 6, 10, False, False, False),      # j_valid 12 < jp 16; K = 36; the input gradient has 3 outputs
    (64, 64, 128, 2, 6, 10, True, True, True),      # M = 120
    (512, 512, 1024, 1, 2, 2, True, True, True),    # M = 4, 8 N tiles; the weight gradient's m_chunk 32 holds 4 pixels
    (1024, 1024, 512, 2, 2, 4, True, True, True),   # K = 9216
]
DC_IDS = ["3in4-64", "64-128", "512-1024-M4", "1024-512-K9216"]


def _run_double_conv(case, math, label, report, staged=False, mag=1.0):
    from floodgan import ops, pix2pix as P2P, plans as PL
    from floodgan.plans import Slice
    cin, ca, cout, N, H, W, f_f3, w_f3, d_f3 = case
    R = _ref_conv(cin, cout, N, H, W, 3, 1, 1, False, mag)
    X = buf_from(R["x"], 1, "constant", ca)             # zero border 1, zero padding channels: both are read
    P = {"c.weight": _dev(R["w"])}
    errs, kern = {}, {}
    Y = _nan_buf(N, H, W, cout)
    P2P._conv_nb(P, "c", X, 1, 3, 1, Y)                 # as segmentation._double_conv (bias=False)
    kern["fwd"] = ops.LAST_CONV_KERNEL
    _only_wrote(Y, 0, cout)
    errs["fwd"] = nrel(nchw(Y), R["y"])
    if (cin, cout) == (64, 128):                        # into the first half of a bordered 256-channel cat buffer
        cat = _nan_buf(N, H, W, 256, 1)
        P2P._conv_nb(P, "c", X, 1, 3, 1, Slice(cat, 0, 128))
        kern["fwd_slice"] = ops.LAST_CONV_KERNEL
        _only_wrote(cat, 0, 128)
        errs["fwd_slice"] = nrel(nchw(cat, 128), R["y"])
    # backward as segmentation._double_conv_bwd: the output gradient with a zero border 1
    G = buf_from(R["gy"], 1, "constant")
    dw = _nan_like(R["w"])
    ops.wgrad(PL.wgrad_conv(G, X, 1, 3, 1, cout), PL.wmap_wgrad(dw.shape, True, X.c, 3), dw)
    kern["wgrad"] = ops.LAST_WGRAD_KERNEL
    assert bool(torch.isfinite(dw).all())
    errs["wgrad"] = nrel(dw, R["gw"])
    GX = _nan_buf(N, H, W, ca)
    md = PL.wmap_conv_dgrad_s1(dw.shape, G.c)
    ops.conv([PL.conv_problem(G, 1, 3, 1, ops.pack_weight(P["c.weight"], md), md, GX)])
    kern["dgrad"] = ops.LAST_CONV_KERNEL
    _only_wrote(GX, 0, cin)                             # cin = 3: channel 3 of the 4 untouched
    errs["dgrad"] = nrel(nchw(GX, cin), R["gx"])
    assert kern["fwd"] == _fwd_family(math, f_f3 and not staged), kern
    assert kern.get("fwd_slice", kern["fwd"]) == kern["fwd"], kern
    assert kern["wgrad"] == _wgrad_family(math, w_f3), kern
    assert kern["dgrad"] == _fwd_family(math, d_f3 and not staged), kern
    _record(report, "double_conv", DC_IDS[DC_CASES.index(case)], label, errs, kern)


@pytest.mark.parametrize("conv_math", MATHS, indirect=True)
@pytest.mark.parametrize("case", DC_CASES, ids=DC_IDS)
def test_double_conv(case, conv_math, report):
    _run_double_conv(case, conv_math, conv_math, report)


# ------------------------------------------------------------------ the cat's input gradient as two halves

# (I, O, split, N, H, W): both halves have `split` > 32 outputs and jp = 3 * O, a multiple of 32 -> pipelined
SPLIT_CASES = [(128, 64, 64, 2, 6, 10), (1024, 512, 512, 1, 2, 2)]
SPLIT_IDS = ["128-64", "1024-512-M4"]


def _run_split_dgrad(case, math, label, report, staged=False):
    from floodgan import ops, plans as PL
    I, O, split, N, H, W = case
    R = _ref_conv(I, O, N, H, W, 3, 1, 1, False)
    wt = _dev(R["w"])
    g_t = buf_from(R["gy"], 1, "constant")
    halves, probs = [], []
    for c0 in (0, split):                                # as segmentation._double_conv_bwd(split=...)
        g_h = _nan_buf(N, H, W, split)
        m = PL.wmap_conv_dgrad_s1_part(wt.shape, g_t.c, c0, split)
        probs.append(PL.conv_problem(g_t, 1, 3, 1, ops.pack_weight(wt, m), m, g_h))
        halves.append(g_h)
    ops.conv(probs)
    kern = {"dgrad": ops.LAST_CONV_KERNEL}
    errs = {}
    for c0, g_h in zip((0, split), halves):
        _only_wrote(g_h, 0, split)
        errs[f"dgrad[{c0}:]"] = nrel(nchw(g_h), R["gx"][:, c0:c0 + split])
    assert kern["dgrad"] == _fwd_family(math, not staged), kern
    _record(report, "split_dgrad", SPLIT_IDS[SPLIT_CASES.index(case)], label, errs, kern)


@pytest.mark.parametrize("conv_math", MATHS, indirect=True)
@pytest.mark.parametrize("case", SPLIT_CASES, ids=SPLIT_IDS)
def test_split_input_gradient(case, conv_math, report):
    _run_split_dgrad(case, conv_math, conv_math, report)


# ------------------------------------------------------------------ ConvTranspose2d(2, 2, 0)

# (cin, cout, N, H, W): phases of one tap (kh = 1, K = cin = jp) with cout > 32 outputs -> pipelined; the weight
# gradient has n_a = cin >= 64 rows and K = 4 cout >= 256; the input gradient is one k = 2, stride-2 conv, jp = 2 cout
T2_CASES = [(1024, 512, 1, 2, 2), (128, 64, 2, 6, 10)]
T2_IDS = ["1024-512-M4", "128-64-K128"]


def _run_convT2(case, math, label, report, staged=False, mag=1.0):
    from floodgan import ops, plans as PL, segmentation as SEG
    from floodgan.plans import Slice
    cin, c, N, H, W = case
    R = _ref_convT(cin, c, N, H, W, 2, 0, mag)
    P = {"up.weight": _dev(R["w"]), "up.bias": _dev(R["b"])}
    X = buf_from(R["x"], 1, "constant")
    cat = _nan_buf(N, 2 * H, 2 * W, 2 * c, 1)            # the decoder level's cat buffer: this conv owns [c, 2c)
    SEG._convT2(P, "up", X, Slice(cat, c, c))
    kern = {"fwd": ops.LAST_CONV_KERNEL}
    _only_wrote(cat, c, c)
    errs = {"fwd": nrel(cat.interior()[..., c:].permute(0, 3, 1, 2).cpu(), R["y"])}
    # backward as segmentation._convT2_bwd: the output gradient without a border
    wt = P["up.weight"]
    g_y = buf_from(R["gy"], 0, "constant")
    dw = _nan_like(R["w"])
    ops.wgrad(PL.wgrad_convT(X, g_y, 2, 0, cin), PL.wmap_wgrad(wt.shape, True, g_y.c, 2), dw)
    kern["wgrad"] = ops.LAST_WGRAD_KERNEL
    assert bool(torch.isfinite(dw).all())
    errs["wgrad"] = nrel(dw, R["gw"])
    g_x = _nan_buf(N, H, W, cin)
    m = PL.wmap_convT_dgrad(wt.shape, g_y.c)
    ops.conv([PL.conv_problem(g_y, 0, 2, 2, ops.pack_weight(wt, m), m, g_x)])
    kern["dgrad"] = ops.LAST_CONV_KERNEL
    _only_wrote(g_x, 0, cin)
    errs["dgrad"] = nrel(nchw(g_x), R["gx"])
    assert kern["fwd"] == kern["dgrad"] == _fwd_family(math, not staged), kern
    assert kern["wgrad"] == _wgrad_family(math, True), kern
    _record(report, "convT2", T2_IDS[T2_CASES.index(case)], label, errs, kern)


@pytest.mark.parametrize("conv_math", MATHS, indirect=True)
@pytest.mark.parametrize("case", T2_CASES, ids=T2_IDS)
def test_convT2(case, conv_math, report):
    _run_convT2(case, conv_math, conv_math, report)


# ------------------------------------------------------------------ Pix2Pix down conv: 4x4, stride 2, pad 1

# (cin, cout, N, H, W): 2 x 2 -> 1 x 1, M = N rows; K = 16 * 512 = 8192; every kernel is the pipelined one in f16x3
DOWN_CASES = [(512, 512, 1, 2, 2), (512, 512, 2, 2, 2)]
DOWN_IDS = ["512-512-N1", "512-512-N2"]


def _run_down(case, math, label, report, staged=False):
    from floodgan import ops, pix2pix as P2P, plans as PL
    cin, cout, N, H, W = case
    R = _ref_conv(cin, cout, N, H, W, 4, 2, 1, True)
    P = {"d.weight": _dev(R["w"]), "d.bias": _dev(R["b"])}
    wd = P["d.weight"]
    X = buf_from(R["x"], 1, "constant")
    Y = _nan_buf(N, H // 2, W // 2, cout)
    P2P._conv_nb(P, "d", X, 1, 4, 2, Y)
    kern = {"fwd": ops.LAST_CONV_KERNEL}
    _only_wrote(Y, 0, cout)
    errs = {"fwd": nrel(nchw(Y), R["y"])}
    G = buf_from(R["gy"], 1, "constant")                 # as pix2pix.gen_backward's g_c: zero border 1
    dw = _nan_like(R["w"])
    ops.wgrad(PL.wgrad_conv(G, X, 1, 4, 2, cout), PL.wmap_wgrad(wd.shape, True, X.c, 4), dw)
    kern["wgrad"] = ops.LAST_WGRAD_KERNEL
    assert bool(torch.isfinite(dw).all())
    errs["wgrad"] = nrel(dw, R["gw"])
    gx = _nan_buf(N, H, W, cin)
    maps = PL.phase_maps(wd.shape, 4, 1, G.c)            # the four-phase input gradient
    ops.conv(PL.phase_problems(G, wd.shape, 4, 1, gx, [ops.pack_weight(wd, mm) for mm, _, _ in maps], maps))
    kern["dgrad"] = ops.LAST_CONV_KERNEL
    _only_wrote(gx, 0, cin)
    errs["dgrad"] = nrel(nchw(gx), R["gx"])
    assert kern["fwd"] == kern["dgrad"] == _fwd_family(math, not staged), kern
    assert kern["wgrad"] == _wgrad_family(math, True), kern
    _record(report, "down4", DOWN_IDS[DOWN_CASES.index(case)], label, errs, kern)


@pytest.mark.parametrize("conv_math", MATHS, indirect=True)
@pytest.mark.parametrize("case", DOWN_CASES, ids=DOWN_IDS)
def test_down_conv(case, conv_math, report):
    _run_down(case, conv_math, conv_math, report)


# ------------------------------------------------------------------ ConvTranspose2d(4, 2, 1)

# (cin, cout, c_alloc of the output, N, H, W, pipelined forward / weight gradient / input gradient?)
T4_CASES = [
    (512, 512, 512, 2, 1, 1, True, True, True),     # phases read a 1 x 1 input and its zero border; M = N per phase
    (1024, 512, 512, 1, 2, 4, True, True, True),    # K = 4096 per phase
    # the outermost up conv: 3 outputs in 4 channels (<= 32 outputs: register-staged); the weight gradient gathers the
    # 4-channel gradient, K = 64 < 256; the input gradient is a stride-2 conv over it, jp = 16
    (128, 3, 4, 2, 6, 10, False, False, False),
]
T4_IDS = ["512-512-1x1", "1024-512-K4096", "128-3in4"]


def _run_convT4(case, math, label, report, staged=False, mag=1.0):
    from floodgan import ops, pix2pix as P2P, plans as PL
    cin, cout, ca, N, H, W, f_f3, w_f3, d_f3 = case
    R = _ref_convT(cin, cout, N, H, W, 4, 1, mag)
    P = {"up.weight": _dev(R["w"]), "up.bias": _dev(R["b"])}
    w = P["up.weight"]
    X = buf_from(R["x"], 1, "constant")
    Y = _nan_buf(N, 2 * H, 2 * W, ca)
    P2P._convT4(P, "up", X, Y)
    kern = {"fwd": ops.LAST_CONV_KERNEL}
    _only_wrote(Y, 0, cout)
    errs = {"fwd": nrel(nchw(Y, cout), R["y"])}
    # backward as pix2pix.gen_backward: the output gradient with a zero border 1 (and zero padding channels)
    G = buf_from(R["gy"], 1, "constant", ca)
    dw = _nan_like(R["w"])
    ops.wgrad(PL.wgrad_convT(X, G, 4, 1, cin), PL.wmap_wgrad(w.shape, True, G.c, 4), dw)
    kern["wgrad"] = ops.LAST_WGRAD_KERNEL
    assert bool(torch.isfinite(dw).all())
    errs["wgrad"] = nrel(dw, R["gw"])
    g_x = _nan_buf(N, H, W, cin)
    m = PL.wmap_convT_dgrad(w.shape, G.c)
    ops.conv([PL.conv_problem(G, 1, 4, 2, ops.pack_weight(w, m), m, g_x)])
    kern["dgrad"] = ops.LAST_CONV_KERNEL
    _only_wrote(g_x, 0, cin)
    errs["dgrad"] = nrel(nchw(g_x), R["gx"])
    assert kern["fwd"] == _fwd_family(math, f_f3 and not staged), kern
    assert kern["wgrad"] == _wgrad_family(math, w_f3), kern
    assert kern["dgrad"] == _fwd_family(math, d_f3 and not staged), kern
    _record(report, "convT4", T4_IDS[T4_CASES.index(case)], label, errs, kern)


@pytest.mark.parametrize("conv_math", MATHS, indirect=True)
@pytest.mark.parametrize("case", T4_CASES, ids=T4_IDS)
def test_convT4(case, conv_math, report):
    _run_convT4(case, conv_math, conv_math, report)


# ------------------------------------------------------------------ beyond the three maths

_WIDE = ([(_run_double_conv, c, f"double_conv-{i}") for c, i in zip(DC_CASES, DC_IDS)]
         + [(_run_split_dgrad, c, f"split_dgrad-{i}") for c, i in zip(SPLIT_CASES, SPLIT_IDS)]
         + [(_run_convT2, c, f"convT2-{i}") for c, i in zip(T2_CASES, T2_IDS)]
         + [(_run_down, c, f"down4-{i}") for c, i in zip(DOWN_CASES, DOWN_IDS)]
         + [(_run_convT4, c, f"convT4-{i}") for c, i in zip(T4_CASES, T4_IDS) if c[1] >= 64])


@pytest.mark.parametrize("run,case", [(r, c) for r, c, _ in _WIDE], ids=[i for _, _, i in _WIDE])
def test_wide_cases_f16x3_register_staged(run, case, report):
    """every case with >= 64 outputs once more in f16x3 with the pipelined forward kernel off (fg_set_f3_tile(-2)):
    the register-staged f16x3 kernel is what runs wherever fgc::f3_takes declines"""
    with _f16x3(f3_tile=-2):
        run(case, "f16x3", "f16x3/staged", report, staged=True)


@pytest.mark.parametrize("run,case", [(_run_double_conv, DC_CASES[3]), (_run_convT2, T2_CASES[0]),
                                      (_run_convT4, T4_CASES[1])],
                         ids=["double_conv-1024-512", "convT2-1024-512", "convT4-1024-512"])
def test_gradient_like_magnitudes_f16x3(run, case, report):
    """activations, biases and gradients x 1e-9 (what the deep levels' gradients look like) in f16x3: the operand
    scales come from the absmax slots, so the error relative to fp64 must not depend on the magnitude"""
    with _f16x3():
        run(case, "f16x3", "f16x3/1e-9", report, mag=1e-9)


# ------------------------------------------------------------------ the bound bites

def _tap_guard(y, y_perturbed):
    e = nrel(y_perturbed, y)
    assert e >= 100 * KTOL, f"one zeroed kernel tap moves the output by only {e:.2e}: the case is too big to notice"
    return e


@pytest.mark.parametrize("case", DC_CASES + [(I, I, O, N, H, W) for I, O, _, N, H, W in SPLIT_CASES] + DOWN_CASES,
                         ids=[f"double_conv-{i}" for i in DC_IDS] + [f"split_dgrad-{i}" for i in SPLIT_IDS]
                         + [f"down4-{i}" for i in DOWN_IDS])
def test_one_zeroed_tap_exceeds_the_bound_conv(case):
    """CPU only: zeroing one kernel tap (all input channels) of one output channel in the fp64 reference moves the
    forward output (for the split case: the input gradient) by at least 100 x KTOL, so a kernel that dropped or
    misplaced one tap of one channel could not pass"""
    if len(case) == 9:
        cin, _, cout, N, H, W = case[:6]
        k, s, bias = 3, 1, False
    elif len(case) == 6:
        cin, _, cout, N, H, W = case
        k, s, bias = 3, 1, False
    else:
        cin, cout, N, H, W = case
        k, s, bias = 4, 2, True
    R = _ref_conv(cin, cout, N, H, W, k, s, 1, bias)
    w = R["w"].clone()
    w[cout // 2, :, 1, 1] = 0.0                      # tap (1, 1) meets a real pixel at every output position here
    if len(case) == 6:
        xr = R["x"].clone().requires_grad_(True)
        (gx,) = torch.autograd.grad(F.conv2d(xr, w, None, stride=s, padding=1), xr, R["gy"])
        _tap_guard(R["gx"], gx)
    else:
        _tap_guard(R["y"], F.conv2d(R["x"], w, R["b"], stride=s, padding=1))


@pytest.mark.parametrize("case,k,p", [(c, 2, 0) for c in T2_CASES] + [(c[:2] + c[3:6], 4, 1) for c in T4_CASES],
                         ids=[f"convT2-{i}" for i in T2_IDS] + [f"convT4-{i}" for i in T4_IDS])
def test_one_zeroed_tap_exceeds_the_bound_convT(case, k, p):
    """the same guard for the transposed convs: one tap of one output channel (all input channels)"""
    cin, cout, N, H, W = case
    R = _ref_convT(cin, cout, N, H, W, k, p)
    w = R["w"].clone()
    w[:, cout // 2, 1, 1] = 0.0
    _tap_guard(R["y"], F.conv_transpose2d(R["x"], w, R["b"], stride=2, padding=p))
