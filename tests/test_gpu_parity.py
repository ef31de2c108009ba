"""GPU parity of the HIP path (libfloodgan via the C-ABI) against the CPU oracle / torch-CPU
fp64 references.  Tolerance: norm-relative 1e-3 per tensor for the network and the step
(BASELINE.json north_star "within 1e-3 relative fp32 tolerance"); kernels are held to 1e-5."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import paired_attention as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
KTOL = 1e-5     # single kernels vs fp64
NTOL = 1e-3     # network / step (north-star tolerance)


MATHS = ["fp32", "bf16x6", "f16x3"]


@pytest.fixture
def conv_math(request):
    """Run a test under one conv math, restoring the library default afterwards."""
    from floodgan import _lib as L
    prev = L.get_conv_math()
    L.set_conv_math(request.param)
    yield request.param
    L.set_conv_math(prev)


def nrel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from floodgan import _lib as L
    L.load()
    L.check(L.load().fg_device_ok(), "device_ok")


def buf_from(x_nchw, pad, mode, c_alloc=None):
    from floodgan.plans import Buf
    n, c, h, w = x_nchw.shape
    c_alloc = c_alloc or c
    xp = F.pad(x_nchw, (pad,) * 4, mode=mode) if pad else x_nchw
    nhwc = torch.zeros(n, h + 2 * pad, w + 2 * pad, c_alloc, dtype=torch.float32)
    nhwc[..., :c] = xp.float().permute(0, 2, 3, 1)
    return Buf(nhwc.reshape(-1).to(DEV), n, h, w, c_alloc, pad)


def nchw(B, c=None):
    c = c or B.c
    return B.interior()[..., :c].permute(0, 3, 1, 2).cpu()


# ------------------------------------------------------------------ conv engine

def _fold_cpu(gpad, p):
    """adjoint of reflect padding on the CPU (test helper)"""
    n, c, hp, wp = gpad.shape
    x = torch.zeros(n, c, hp - 2 * p, wp - 2 * p, dtype=gpad.dtype, requires_grad=True)
    (g,) = torch.autograd.grad(F.pad(x, (p,) * 4, mode="reflect"), x, gpad)
    return g


CONV_CASES = [(9, 64, 7, 1, 3, "reflect", 24), (64, 128, 3, 2, 1, "constant", 20), (256, 256, 3, 1, 1, "reflect", 12),
              (64, 27, 7, 1, 3, "reflect", 16), (64, 10, 1, 1, 0, "constant", 16), (12, 64, 4, 2, 1, "constant", 32),
              (128, 256, 4, 2, 1, "constant", 16), (256, 512, 4, 1, 1, "constant", 9), (512, 1, 4, 1, 1, "constant", 9),
              # 1x1 head at 96^2: the weight gradient splits >= 32 ways over 640 elements (split-parallel reduce)
              (64, 10, 1, 1, 0, "constant", 96)]


@pytest.mark.parametrize("conv_math", MATHS, indirect=True)
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fwd_wgrad_dgrad(case, conv_math):
    """every conv geometry of the step: forward, weight gradient, input gradient vs fp64, in
    each conv math (the f16x3 case also at gradient-like magnitudes: operands x 1e-9)"""
    from floodgan import ops, plans as PL
    from floodgan.plans import Buf
    cin, cout, k, s, p, mode, H = case
    torch.manual_seed(1)
    mag = 1e-9 if conv_math == "f16x3" and cin == 256 else 1.0
    x = torch.randn(2, cin, H, H, dtype=torch.float64) * mag
    w = (torch.randn(cout, cin, k, k, dtype=torch.float64) * 0.05).requires_grad_(True)
    b = torch.randn(cout, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    xin = F.pad(xr, (p,) * 4, mode=mode) if p else xr
    y = F.conv2d(xin, w, b * mag, stride=s)
    gy = torch.randn_like(y) * mag
    gx_ref, gw_ref = torch.autograd.grad(y, (xr, w), gy)
    X = buf_from(x, p, mode)
    wd = w.detach().float().to(DEV)
    m = PL.wmap_conv_fwd(wd.shape, X.c)
    Ho = PL.out_size(H, k, s, p)
    Y = Buf.empty(2, Ho, Ho, cout, 0, DEV)
    ops.conv([PL.conv_problem(X, p, k, s, ops.pack_weight(wd, m), m, Y, bias=(b * mag).float().to(DEV))])
    assert nrel(nchw(Y), y) < KTOL
    # weight gradient
    GY = buf_from(gy, 0, "constant")
    dw = torch.empty_like(wd)
    ops.wgrad(PL.wgrad_conv(GY, X, p, k, s, cout), PL.wmap_wgrad(wd.shape, True, X.c, k), dw)
    assert nrel(dw, gw_ref) < KTOL
    # input gradient
    if s == 1:
        if mode == "reflect":
            GYP = buf_from(gy, k - 1, "constant")
            gxp = Buf.empty(2, H + 2 * p, H + 2 * p, cin, 0, DEV)
            md = PL.wmap_conv_dgrad_s1(wd.shape, GYP.c)
            ops.conv([PL.conv_problem(GYP, k - 1, k, 1, ops.pack_weight(wd, md), md, gxp)])
            if cin % 4 == 0:
                gx = Buf.empty(2, H, H, cin, 0, DEV)
                ops.fold_add(gxp, p, None, gx)
            else:   # the fold kernel is float4-wide; this geometry (conv1) never needs it
                torch.cuda.synchronize()
                assert nrel(_fold_cpu(nchw(gxp).double(), p), gx_ref) < KTOL
                return
        else:
            GYP = buf_from(gy, k - 1 - p, "constant")
            gx = Buf.empty(2, H, H, cin, 0, DEV)
            md = PL.wmap_conv_dgrad_s1(wd.shape, GYP.c)
            ops.conv([PL.conv_problem(GYP, k - 1 - p, k, 1, ops.pack_weight(wd, md), md, gx)])
    else:
        GYP = buf_from(gy, 1, "constant")
        gx = Buf.empty(2, H, H, cin, 0, DEV)
        maps = PL.phase_maps(wd.shape, k, p, GYP.c)
        ops.conv(PL.phase_problems(GYP, wd.shape, k, p, gx, [ops.pack_weight(wd, mm) for mm, _, _ in maps], maps))
    torch.cuda.synchronize()
    assert nrel(nchw(gx), gx_ref) < KTOL


@pytest.mark.parametrize("conv_math", MATHS, indirect=True)
@pytest.mark.parametrize("cin,cout,H", [(256, 128, 12), (128, 64, 20)])
def test_convT(cin, cout, H, conv_math):
    from floodgan import ops, plans as PL
    from floodgan.plans import Buf
    torch.manual_seed(2)
    x = torch.randn(2, cin, H, H, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(cin, cout, 3, 3, dtype=torch.float64) * 0.05).requires_grad_(True)
    b = torch.randn(cout, dtype=torch.float64)
    y = F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    gy = torch.randn_like(y)
    gx_ref, gw_ref = torch.autograd.grad(y, (x, w), gy)
    X = buf_from(x.detach(), 1, "constant")
    wd = w.detach().float().to(DEV)
    Y = Buf.empty(2, 2 * H, 2 * H, cout, 0, DEV)
    maps = PL.phase_maps(wd.shape, 3, 1, X.c)
    ops.conv(PL.phase_problems(X, wd.shape, 3, 1, Y, [ops.pack_weight(wd, m) for m, _, _ in maps], maps,
                               bias=b.float().to(DEV)))
    assert nrel(nchw(Y), y) < KTOL
    GY = buf_from(gy, 1, "constant")
    dw = torch.empty_like(wd)
    ops.wgrad(PL.wgrad_convT(X, GY, 3, 1, cin), PL.wmap_wgrad(wd.shape, True, GY.c, 3), dw)
    assert nrel(dw, gw_ref) < KTOL
    gx = Buf.empty(2, H, H, cin, 0, DEV)
    m = PL.wmap_convT_dgrad(wd.shape, GY.c)
    ops.conv([PL.conv_problem(GY, 1, 3, 2, ops.pack_weight(wd, m), m, gx)])
    assert nrel(nchw(gx), gx_ref) < KTOL


@pytest.mark.parametrize("persistent,sched,order", [(0, 2, 3), (1, 2, 3), (1, 1, 3), (1, 0, 3), (1, 1, 2),
                                                    (1, 1, 1), (1, 1, 0), (1, 1, 7), (1, 3, 7), (0, 3, 7),
                                                    (1, 3, 15), (3, 3, 15), (1, 3, 31), (3, 3, 31)])
@pytest.mark.parametrize("cfg", [-2, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
@pytest.mark.parametrize("case", [(256, 256, 3, 1, 1, "reflect", 20), (128, 256, 4, 2, 1, "constant", 22),
                                  (64, 128, 3, 2, 1, "constant", 30), (256, 512, 4, 1, 1, "constant", 11),
                                  (128, 64, 3, 1, 1, "constant", 21)])
def test_conv_f3_tiles(case, cfg, persistent, sched, order):
    """the pipelined f16x3 forward kernel (conv_f3.hip) in every tile config, stage schedule and
    k-walk order, ragged M / N tiles included, against fp64 -- and the register-staged kernel it
    replaces (cfg -2)"""
    from floodgan import _lib as L, ops, plans as PL
    from floodgan.plans import Buf
    cin, cout, k, s, p, mode, H = case
    prev = L.get_conv_math()
    L.set_conv_math("f16x3")
    try:
        L.set_f3_tile(cfg)
        L.load().fg_set_f3_persistent(persistent)
        L.load().fg_set_f3_sched(sched)
        L.load().fg_set_f3_order(order)
        torch.manual_seed(3)
        x = torch.randn(3, cin, H, H, dtype=torch.float64)
        w = torch.randn(cout, cin, k, k, dtype=torch.float64) * 0.05
        b = torch.randn(cout, dtype=torch.float64)
        xin = F.pad(x, (p,) * 4, mode=mode) if p else x
        y = F.conv2d(xin, w, b, stride=s)
        X = buf_from(x, p, mode)
        wd = w.float().to(DEV)
        m = PL.wmap_conv_fwd(wd.shape, X.c)
        Ho = PL.out_size(H, k, s, p)
        Y = Buf.empty(3, Ho, Ho, cout, 0, DEV)
        ops.conv([PL.conv_problem(X, p, k, s, ops.pack_weight(wd, m), m, Y, bias=b.float().to(DEV),
                                  act=1)])
        torch.cuda.synchronize()
        assert nrel(nchw(Y), torch.relu(y)) < KTOL
    finally:
        L.set_f3_tile(-1)
        L.load().fg_set_f3_persistent(1)
        L.load().fg_set_f3_sched(-1)
        L.load().fg_set_f3_order(L.F3_ORDER_DEFAULT)
        L.set_conv_math(prev)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
@pytest.mark.parametrize("case", [(32, 128, 1, 1, 0, "constant", 40),    # K = 32: one k chunk per tile (nkt < NS)
                                  (64, 64, 1, 1, 0, "constant", 37),     # K = 64: two chunks, ragged M
                                  (32, 256, 3, 1, 1, "reflect", 24)])    # K = 288: several chunks per tile
def test_conv_f3_persistent_bit_exact(case, cfg):
    """the tile-crossing stream of the persistent conv_f3 kernel (a few workgroups each walk many tiles: the next
    tile's stages are issued over the previous tile's epilogue stores, and wait_stage counts those NST stores into
    its vmcnt) gives output bit-identical to one workgroup per tile -- short-K convs (one k chunk per tile, fewer
    than the ring depth) are where a too-loose stage wait would read a stage before its DMA landed"""
    from floodgan import _lib as L, ops, plans as PL
    from floodgan.plans import Buf
    cin, cout, k, s, p, mode, H = case
    prev = L.get_conv_math()
    L.set_conv_math("f16x3")
    try:
        L.set_f3_tile(cfg)
        torch.manual_seed(17)
        x = torch.randn(3, cin, H, H, dtype=torch.float64)
        w = torch.randn(cout, cin, k, k, dtype=torch.float64) * 0.1
        X = buf_from(x, p, mode)
        wd = w.float().to(DEV)
        m = PL.wmap_conv_fwd(wd.shape, X.c)
        Ho = PL.out_size(H, k, s, p)
        out = {}
        # order bit 3: the freed ring slot refilled before each tile's epilogue stores (the stage waits then count
        # those stores one stage later)
        for order in (7, 15, 31):
            L.load().fg_set_f3_order(order)
            for persistent in (0, 2, 3, 7):
                L.load().fg_set_f3_persistent(persistent)
                Y = Buf.empty(3, Ho, Ho, cout, 0, DEV)
                Y.t.fill_(float("nan"))
                ops.conv([PL.conv_problem(X, p, k, s, ops.pack_weight(wd, m), m, Y,
                                          bias=torch.ones(cout, device=DEV))])
                assert ops.LAST_CONV_KERNEL == "conv_fwd_f3", ops.LAST_CONV_KERNEL
                out[order, persistent] = Y.t.clone()
        torch.cuda.synchronize()
        assert not torch.isnan(out[7, 0]).any()
        for key in out:
            assert torch.equal(out[key], out[key[0], 0]), key
        assert torch.equal(out[15, 0], out[7, 0])   # bit 3 moves no arithmetic (bit 4 moves the reversed rows)
    finally:
        L.set_f3_tile(-1)
        L.load().fg_set_f3_persistent(1)
        L.load().fg_set_f3_order(L.F3_ORDER_DEFAULT)
        L.set_conv_math(prev)


@pytest.mark.parametrize("presplit", [False, True])
def test_conv_f3_tile_height_invariant(presplit):
    """order bit 4 (default): odd 512-row blocks of output rows walk the kernel rows backwards whatever the tile
    height, so every tile config gives a row the same k order -- the outputs of 128-, 256- and 512-row tiles are
    bit-identical, and a sample's values do not depend on the tile config its batch size selects (the batch-8 vs
    batch-1 check of test_bs8_generator_backward_equals_sum_of_bs1_512)"""
    from floodgan import _lib as L, ops, plans as PL
    from floodgan.plans import Buf
    prev = L.get_conv_math()
    L.set_conv_math("f16x3")
    lib = L.load()
    try:
        torch.manual_seed(29)
        cin, cout, H = 64, 128, 40
        c = torch.randn(3, cin, H, H, dtype=torch.float64)
        if presplit:
            cb = buf_from(c, 0, "constant")
            mean, rstd = ops.in_stats(cb)
            X = Buf.empty(3, H, H, cin, 1, DEV)
            ops.in_apply(cb, mean, rstd, 1, None, X, 1, presplit=True)
        else:
            X = buf_from(c, 1, "reflect")
        wd = (torch.randn(cout, cin, 3, 3, dtype=torch.float64) * 0.05).float().to(DEV)
        m = PL.wmap_conv_fwd(wd.shape, cin)
        wp = ops.pack_weight(wd, m)
        out = {}
        for cfg in (3, 6, 9, 10, 11, 12):
            L.set_f3_tile(cfg)
            Y = Buf.empty(3, H, H, cout, 0, DEV)
            ops.conv([PL.conv_problem(X, 1, 3, 1, wp, m, Y)])
            out[cfg] = Y.t.clone()
        torch.cuda.synchronize()
        for cfg in out:
            assert torch.equal(out[cfg], out[3]), cfg
    finally:
        L.set_f3_tile(-1)
        lib.fg_set_f3_order(L.F3_ORDER_DEFAULT)
        L.set_conv_math(prev)


@pytest.mark.parametrize("cfg", [3, 10, 12])
def test_conv_f3_batch_position_invariant(cfg):
    """order bit 4 counts its 512-row blocks from the tile's image when an image holds a whole number of them, so a
    sample's output does not depend on its position in the batch: 32 x 48 images are 1536 rows = 3 x 512,
    so blocks counted from the batch's first row would flip the k order of every second image.  Each image of a
    batch of 3 must equal its own batch-1 launch bit for bit, on 128- and 512-row tiles."""
    from floodgan import _lib as L, ops, plans as PL
    from floodgan.plans import Buf
    prev = L.get_conv_math()
    L.set_conv_math("f16x3")
    try:
        torch.manual_seed(31)
        cin, cout, Hh, Ww = 64, 128, 32, 48
        c = torch.randn(3, cin, Hh, Ww, dtype=torch.float64)
        cb = buf_from(c, 0, "constant")
        mean, rstd = ops.in_stats(cb)
        X = Buf.empty(3, Hh, Ww, cin, 1, DEV)
        ops.in_apply(cb, mean, rstd, 1, None, X, 1, presplit=True)
        wd = (torch.randn(cout, cin, 3, 3, dtype=torch.float64) * 0.05).float().to(DEV)
        m = PL.wmap_conv_fwd(wd.shape, cin)
        wp = ops.pack_weight(wd, m)
        L.set_f3_tile(cfg)
        Y = Buf.empty(3, Hh, Ww, cout, 0, DEV)
        ops.conv([PL.conv_problem(X, 1, 3, 1, wp, m, Y)])
        img = X.t.numel() // 3
        for i in range(3):
            Xi = Buf(X.t[i * img:(i + 1) * img], 1, Hh, Ww, cin, 1)
            ops.adopt(Xi, X)            # the batch's scale slot, the producer's FG_PRESPLIT image
            assert ops.slot_of(Xi) is ops.slot_of(X) and ops.is_presplit(Xi)
            Yi = Buf.empty(1, Hh, Ww, cout, 0, DEV)
            ops.conv([PL.conv_problem(Xi, 1, 3, 1, wp, m, Yi)])
            assert torch.equal(Yi.t.view(-1), Y.t.view(3, -1)[i]), (cfg, i)
    finally:
        L.set_f3_tile(-1)
        L.set_conv_math(prev)


def test_paired_step_under_forced_tile():
    """a whole paired step with a forced tile config (fg_set_f3_tile, a tuning hook): the quad-form launches
    (deconv2, conv2's input gradient) keep their one tile instead of failing, and the pre-update losses
    equal the default dispatch's to rounding"""
    from floodgan import _lib as L
    torch.manual_seed(3)
    x = (torch.rand(2, 9, 64, 64) * 2 - 1).to(DEV)
    y = (torch.rand(2, 3, 64, 64) * 2 - 1).to(DEV)
    ref = _make_model().step_fn(x, y).cpu()
    try:
        for cfg in (4, 11):
            L.set_f3_tile(cfg)
            got = _make_model().step_fn(x, y).cpu()
            assert torch.isfinite(got).all()
            assert (got - ref).abs().max() <= 1e-5 * ref.abs().max(), (cfg, got, ref)
    finally:
        L.set_f3_tile(-1)


@pytest.mark.parametrize("on", [0, 1, 2, 3])
@pytest.mark.parametrize("case", [(256, 256, 3, 1, 1, "reflect", 40), (128, 256, 4, 2, 1, "constant", 34),
                                  (256, 512, 4, 1, 1, "constant", 17), (64, 128, 3, 2, 1, "constant", 36),
                                  (128, 128, 4, 2, 1, "constant", 30),
                                  # 64 output channels (the 64-row tile): the stem 7x7 over 12 channels, a 3x3 64->64
                                  (12, 64, 7, 1, 3, "reflect", 38), (64, 64, 3, 1, 1, "reflect", 33),
                                  # D model.0: 4x4 s2 over 12 channels, K = 192 (the register-staged kernel)
                                  (12, 64, 4, 2, 1, "constant", 40)])
def test_wgrad_f3(case, on):
    """the pipelined f16x3 weight-gradient kernel (conv_wgrad_f3.hip; on=0: the register-staged
    kernel) on multi-split problems with ragged pixel chunks, against fp64"""
    from floodgan import _lib as L, ops, plans as PL
    cin, cout, k, s, p, mode, H = case
    prev = L.get_conv_math()
    L.set_conv_math("f16x3")
    L.set_wgrad_f3(on)
    try:
        torch.manual_seed(5)
        x = torch.randn(3, cin, H, H, dtype=torch.float64)
        w = torch.randn(cout, cin, k, k, dtype=torch.float64) * 0.05
        xin = F.pad(x, (p,) * 4, mode=mode) if p else x
        Ho = PL.out_size(H, k, s, p)
        gy = torch.randn(3, cout, Ho, Ho, dtype=torch.float64) * 1e-5
        gw_ref = torch.nn.grad.conv2d_weight(xin, w.shape, gy, stride=s)
        X = buf_from(x, p, mode)
        GY = buf_from(gy, 0, "constant")
        dw = torch.empty(w.shape, dtype=torch.float32, device=DEV)
        prob = PL.wgrad_conv(GY, X, p, k, s, cout)
        assert prob["splits"] > 1
        ops.wgrad(prob, PL.wmap_wgrad(w.shape, True, X.c, k), dw)
        torch.cuda.synchronize()
        assert nrel(dw, gw_ref) < KTOL
    finally:
        L.set_wgrad_f3(2)
        L.set_conv_math(prev)


@pytest.mark.parametrize("splits,H,W", [(None, 5, 288), (8, 12, 512), (7, 12, 512), (216, 30, 512)])
def test_wgrad_window(splits, H, W):
    """the row-strip content-head weight gradient (fg_conv_wgrad_win): gradient 27(32) channels
    with its 6-wide zero border, input 64 channels reflect-padded by 3, against fp64 and against
    the generic f16x3 weight-gradient kernel.  The split counts walk several 32-px chunks per split across
    column-block, row and image edges: 8 splits (XCD-grouped, 48 chunks each), 7 (the ungrouped mapping, a
    short last split) and the production 216 over 960 chunks (4-5 each); None = the default over 90 chunks"""
    from floodgan import _lib as L, ops, plans as PL
    prev = L.get_conv_math()
    prev_splits = ops.WIN_WGRAD_SPLITS
    L.set_conv_math("f16x3")
    try:
        if splits is not None:
            ops.WIN_WGRAD_SPLITS = splits
        torch.manual_seed(6)
        x = torch.randn(2, 64, H, W, dtype=torch.float64)
        gy = torch.randn(2, 27, H, W, dtype=torch.float64) * 1e-4
        w = torch.zeros(27, 64, 7, 7, dtype=torch.float64)
        gw_ref = torch.nn.grad.conv2d_weight(F.pad(x, (3,) * 4, mode="reflect"), w.shape, gy)
        X = buf_from(x, 3, "reflect")
        GY = buf_from(gy, 6, "constant", c_alloc=32)
        prob = PL.wgrad_conv(GY, X, 3, 7, 1, 27)
        assert ops.wgrad_win_eligible(prob)
        wm = PL.wmap_wgrad(w.shape, True, X.c, 7)
        dw = torch.empty(w.shape, dtype=torch.float32, device=DEV)
        ops.wgrad(prob, wm, dw)
        torch.cuda.synchronize()
        assert nrel(dw, gw_ref) < KTOL
        ops.USE_WIN = False
        dw2 = torch.empty_like(dw)
        ops.wgrad(prob, wm, dw2)
        torch.cuda.synchronize()
        assert nrel(dw2, gw_ref) < KTOL
    finally:
        ops.USE_WIN = True
        ops.WIN_WGRAD_SPLITS = prev_splits
        L.set_conv_math(prev)


@pytest.mark.parametrize("H,N,splits", [(64, 2, None), (128, 2, None), (128, 1, 4), (192, 1, 3)])
def test_stem_wgrad_strips(H, N, splits):
    """the stem's weight-gradient kernel (conv_stem.hip: 7x7 over the reflect-padded 9-channel input, 64
    outputs; 64-px strips of `rows` output rows per workgroup walking an 8-row LDS ring) against fp64 at
    1 .. 192 rows per split, 1 .. 3 strips per image (models/model_architectures.py:312, :342-343)"""
    from floodgan import _lib as L, ops, plans as PL
    prev, prev_s = L.get_conv_math(), PL.STEM_SPLITS
    L.set_conv_math("f16x3")
    try:
        if splits is not None:
            PL.STEM_SPLITS = splits
        torch.manual_seed(11)
        x = torch.randn(N, 9, H, H, dtype=torch.float64)
        gy = torch.randn(N, 64, H, H, dtype=torch.float64) * 1e-3
        w = torch.zeros(64, 9, 7, 7, dtype=torch.float64)
        gw_ref = torch.nn.grad.conv2d_weight(F.pad(x, (3,) * 4, mode="reflect"), w.shape, gy)
        X = buf_from(x, 3, "reflect")
        GY = buf_from(gy, 0, "constant")
        prob = PL.wgrad_conv(GY, X, 3, 7, 1, 64)
        layout = PL.stem_wgrad_layout(prob)
        assert layout is not None and (splits is None or layout[0] == splits)
        dw = torch.empty(w.shape, dtype=torch.float32, device=DEV)
        ops.wgrad(prob, PL.wmap_wgrad(w.shape, True, X.c, 7), dw)
        assert ops.LAST_WGRAD_KERNEL == "stem_wgrad", ops.LAST_WGRAD_KERNEL
        torch.cuda.synchronize()
        assert nrel(dw, gw_ref) < KTOL
    finally:
        PL.STEM_SPLITS = prev_s
        L.set_conv_math(prev)


@pytest.mark.parametrize("H,N", [(64, 2), (128, 2), (192, 1)])
def test_stem_fwd_strips(H, N):
    """the stem's forward kernel (conv_stem.hip: 7x7 over the reflect-padded 9-channel input, 64 outputs + bias,
    weights resident in registers, 64-px strips over an 8-row LDS ring) against fp64, with and without the
    InstanceNorm statistics epilogue (models/model_architectures.py:312, :342-343)"""
    from floodgan import _lib as L, ops, plans as PL
    from floodgan.plans import Buf
    prev = L.get_conv_math()
    L.set_conv_math("f16x3")
    try:
        torch.manual_seed(12)
        x = torch.rand(N, 9, H, H, dtype=torch.float64) * 2 - 1
        w = torch.randn(64, 9, 7, 7, dtype=torch.float64) * 0.05
        b = torch.randn(64, dtype=torch.float64) * 0.1
        ref = F.conv2d(F.pad(x, (3,) * 4, mode="reflect"), w, b)
        X = buf_from(x, 3, "reflect")
        wd = w.float().to(DEV)
        m = PL.wmap_conv_fwd(wd.shape, X.c)
        for stats in (False, True):
            Y = Buf.empty(N, H, H, 64, 0, DEV)
            st = ops.conv([PL.conv_problem(X, 3, 7, 1, ops.pack_weight(wd, m), m, Y, bias=b.float().to(DEV))],
                          in_stats=stats)
            assert ops.LAST_CONV_KERNEL == "stem_fwd", ops.LAST_CONV_KERNEL
            torch.cuda.synchronize()
            assert nrel(nchw(Y), ref) < KTOL
            if stats:
                assert st is not None
                mu = ref.mean(dim=(2, 3))
                var = ref.var(dim=(2, 3), unbiased=False)
                assert nrel(st[0].view(N, 64), mu) < KTOL
                assert nrel(st[1].view(N, 64), (var + 1e-5).rsqrt()) < KTOL
    finally:
        L.set_conv_math(prev)


@pytest.mark.parametrize("case,env", [("content_fwd", {}), ("content_dgrad", {}), ("content_dgrad_512", {})])
def test_conv_window(case, env, monkeypatch):
    """the row-strip window kernel (fg_conv_win) on the content-head geometries -- 7x7 over 64
    channels -> 27, and its input gradient 27(32) -> 64 over the 6-bordered gradient -- with
    output rows of 256+ px (two-segment tiles, ragged last tile) against fp64; the forward on its two-workgroup
    channel-half kernel, the input gradient on its two-workgroup LDS-DMA kernel"""
    from floodgan import _lib as L, ops, plans as PL
    from floodgan.plans import Buf
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prev = L.get_conv_math()
    L.set_conv_math("f16x3")
    try:
        torch.manual_seed(4)
        if case == "content_fwd":
            cin, cout, H, W = 64, 27, 6, 300
            x = torch.randn(2, cin, H, W, dtype=torch.float64)
            w = torch.randn(cout, cin, 7, 7, dtype=torch.float64) * 0.05
            b = torch.randn(cout, dtype=torch.float64)
            y = F.conv2d(F.pad(x, (3,) * 4, mode="reflect"), w, b)
            X = buf_from(x, 3, "reflect")
            wd = w.float().to(DEV)
            m = PL.wmap_conv_fwd(wd.shape, X.c)
            Y = Buf.empty(2, H, W, 32, 0, DEV)
            prob = PL.conv_problem(X, 3, 7, 1, ops.pack_weight(wd, m), m, Y, bias=b.float().to(DEV))
            ref = y
        else:
            # dgrad: gy has 27 (alloc 32) channels, output 64 over the 6-wider padded domain
            cin, cout, H, W = (64, 27, 5, 290) if case == "content_dgrad" else (64, 27, 3, 515)
            gy = torch.randn(2, cout, H, W, dtype=torch.float64) * 1e-6
            w = torch.randn(cout, cin, 7, 7, dtype=torch.float64) * 0.05
            # gradient w.r.t. the 3-padded input = full correlation of gy with the flipped kernel
            xp = torch.zeros(2, cin, H + 6, W + 6, dtype=torch.float64, requires_grad=True)
            (ref,) = torch.autograd.grad(F.conv2d(xp, w), xp, gy)
            GYP = buf_from(gy, 6, "constant", c_alloc=32)
            wd = w.float().to(DEV)
            md = PL.wmap_conv_dgrad_s1(wd.shape, GYP.c)
            Y = Buf.empty(2, H + 6, W + 6, cin, 0, DEV)
            prob = PL.conv_problem(GYP, 6, 7, 1, ops.pack_weight(wd, md), md, Y)
        # the step routes both here (the input gradient since round 2: 1.58 vs 1.67 ms on the pipelined
        # im2col kernel at bs 8, profiles/round2/r2v_content_dgrad_win.log); the pipelined path is checked below
        assert ops.win_eligible(prob)
        ops.conv_win(prob)
        torch.cuda.synchronize()
        assert nrel(nchw(Y, ref.shape[1]), ref) < KTOL
        # the epilogue's accumulate and activation paths: Y += LeakyReLU(conv) over the first result
        first = nchw(Y, ref.shape[1]).double()
        ops.conv_win(dict(prob, accumulate=1, act=L.FG_ACT_LRELU))
        torch.cuda.synchronize()
        assert nrel(nchw(Y, ref.shape[1]), first + F.leaky_relu(ref, 0.2)) < KTOL
        ops.USE_WIN = False
        Y.t.zero_()
        ops.conv([prob])
        torch.cuda.synchronize()
        assert nrel(nchw(Y, ref.shape[1]), ref) < KTOL
    finally:
        ops.USE_WIN = True
        L.set_conv_math(prev)


@pytest.mark.parametrize("ctot,c0,cn,H,W,acc", [(12, 9, 3, 64, 64, True), (12, 9, 3, 256, 130, False),
                                               (4, 0, 4, 34, 200, True), (6, 2, 1, 18, 18, False)])
def test_d0_input_grad(ctot, c0, cn, H, W, acc):
    """the PatchGAN model.0 input gradient restricted to input channels c0 .. c0+cn-1 (fg_d0_input_grad, exact fp32;
    the G step's dL/d(fake)) against fp64 autograd of Conv2d(ctot, 64, 4, 2, 1), written and accumulated into an
    NCHW tensor, partial 64-column blocks included, and against the engine's restricted transposed conv"""
    from floodgan import executor as X, ops
    torch.manual_seed(31)
    N = 2
    x = torch.randn(N, ctot, H, W, dtype=torch.float64, requires_grad=True)
    w = torch.randn(64, ctot, 4, 4, dtype=torch.float64) * 0.05
    e = F.conv2d(x, w, stride=2, padding=1)
    gy = torch.randn_like(e)
    (gx,) = torch.autograd.grad(e, x, gy)
    G = buf_from(gy, 1, "constant")
    base = torch.randn(N, cn + 1, H, W, device=DEV)
    y = base.clone()
    wd = w.float().to(DEV).contiguous()
    ops.d0_input_grad(G, wd, c0, cn, y, acc)
    torch.cuda.synchronize()
    ref = gx[:, c0:c0 + cn] + (base[:, :cn].double().cpu() if acc else 0)
    assert nrel(y[:, :cn].double().cpu(), ref) < 1e-6
    assert torch.equal(y[:, cn:], base[:, cn:])               # channels past cn untouched
    # the engine's restricted 4-phase transposed conv of the same gradient (the FLOODGAN_D0_DGRAD=0 path)
    y2 = base.clone()
    X._dgrad_s2({"model.0.weight": wd}, "model.0", G, 4, y_nchw=(y2.view(-1), y2.shape[1], H, W), n_base=c0, n_out=cn,
                accumulate=int(acc))
    torch.cuda.synchronize()
    assert nrel(y2[:, :cn].double().cpu(), ref) < KTOL


@pytest.mark.parametrize("N,H,W,n_out,xpad", [(2, 20, 37, 10, 0), (3, 9, 64, 10, 1), (1, 5, 7, 16, 0), (2, 96, 96, 3, 0)])
def test_conv1x1_head(N, H, W, n_out, xpad):
    """the attention head's 1x1 conv in fp32 FMA (fg_conv1x1_*): forward (pad channels written as 0), input
    gradient (the gradient's padding channels NaN: never read), weight + bias gradients (written and accumulated)
    against fp64, ragged last tiles; the forward in lane form"""
    from floodgan import _lib as L, ops
    from floodgan.plans import Buf
    torch.manual_seed(21)
    x = torch.randn(N, 64, H, W, dtype=torch.float64)
    w = (torch.randn(n_out, 64, 1, 1, dtype=torch.float64) * 0.1).requires_grad_(True)
    b = torch.randn(n_out, dtype=torch.float64, requires_grad=True)
    xr = x.clone().requires_grad_(True)
    y = F.conv2d(xr, w, b)
    gy = torch.randn_like(y)
    gx_ref, gw_ref, gb_ref = torch.autograd.grad(y, (xr, w, b), gy)
    X = buf_from(x, xpad, "constant")
    wd, bd = w.detach().float().to(DEV), b.detach().float().to(DEV)
    Y = Buf.empty(N, H, W, 16, 0, DEV)
    Y.t.fill_(float("nan"))
    ops.conv1x1_fwd(X, wd, bd, n_out, Y)
    torch.cuda.synchronize()
    assert nrel(nchw(Y, n_out), y) < KTOL
    if n_out < 16:
        assert float(Y.nhwc()[..., n_out:].abs().max()) == 0.0
    GY = buf_from(gy, 0, "constant", c_alloc=16)
    if n_out < 16:
        GY.nhwc()[..., n_out:] = float("nan")
    GX = Buf.empty(N, H, W, 64, 0, DEV)
    ops.conv1x1_dgrad(GY, wd, n_out, GX)
    dw = torch.full(w.shape, 3.0, device=DEV)
    db = torch.full((n_out,), -2.0, device=DEV)
    ops.conv1x1_wgrad(GY, X, n_out, dw, db)
    torch.cuda.synchronize()
    assert nrel(nchw(GX), gx_ref) < KTOL
    assert nrel(dw, gw_ref) < KTOL and nrel(db, gb_ref) < KTOL
    ops.conv1x1_wgrad(GY, X, n_out, dw, db, accumulate=True)
    torch.cuda.synchronize()
    assert nrel(dw, 2 * gw_ref) < KTOL and nrel(db, 2 * gb_ref) < KTOL


@pytest.mark.parametrize("H", [11, 40])
def test_disc_head_n1(H):
    """model.11 (Conv2d(512, 1, 4, 1, 1)): the fp32 FMA forward and weight-gradient kernels vs fp64 (H 40: output
    rows of 39 px, a ragged last quad)"""
    from floodgan import ops, plans as PL
    from floodgan.plans import Buf
    torch.manual_seed(7)
    N = 3
    x = torch.randn(N, 512, H, H, dtype=torch.float64)
    w = torch.randn(1, 512, 4, 4, dtype=torch.float64) * 0.02
    b = torch.randn(1, dtype=torch.float64)
    y = F.conv2d(F.pad(x, (1,) * 4), w, b)
    gy = torch.randn_like(y)
    gw_ref = torch.nn.grad.conv2d_weight(F.pad(x, (1,) * 4), w.shape, gy)
    X = buf_from(x, 1, "constant")
    out = torch.empty(N, 1, H - 1, H - 1, dtype=torch.float32, device=DEV)
    ops.conv_n1_fwd(X, w.float().to(DEV), b.float().to(DEV), out)
    G = Buf.zeros(N, H - 1, H - 1, 1, 3, DEV)
    G.interior().copy_(gy.float().permute(0, 2, 3, 1))
    dw = torch.empty(1, 512, 4, 4, dtype=torch.float32, device=DEV)
    ops.conv_n1_wgrad(X, G, PL.wmap_wgrad(w.shape, True, 512, 4), dw)
    torch.cuda.synchronize()
    assert nrel(out, y) < KTOL
    assert nrel(dw, gw_ref) < KTOL


# ------------------------------------------------------------------ instance norm

@pytest.mark.parametrize("act,fold,residual,C,gadd", [(1, 0, False, 64, False), (2, 0, False, 64, False),
                                                       (0, 0, True, 64, False), (1, 1, False, 64, False),
                                                       (1, 3, False, 64, False), (1, 1, False, 256, True),
                                                       (2, 1, False, 16, True), (1, 3, False, 32, True),
                                                       (0, 0, False, 128, True)])
def test_instnorm_fwd_bwd(act, fold, residual, C, gadd):
    """IN forward (stats, apply with activation / residual / padding) and backward (fold of the
    reflect-pad gradient, the added residual gradient `gadd`) against fp64 autograd"""
    from floodgan import ops
    from floodgan.plans import Buf
    torch.manual_seed(3)
    H = 20
    c = (torch.randn(2, C, H, H, dtype=torch.float64) * 2 + 0.7).requires_grad_(True)
    r = torch.randn(2, C, H, H, dtype=torch.float64)
    y = F.instance_norm(c, eps=1e-5)
    y = F.relu(y) if act == 1 else (F.leaky_relu(y, 0.2) if act == 2 else y)
    if residual:
        y = y + r
    pad_mode = "reflect" if fold else "constant"
    yp = F.pad(y, (max(fold, 1),) * 4, mode=pad_mode if fold else "constant")
    gy = torch.randn_like(yp)
    if gadd:      # a second gradient on the (unpadded) block output, e.g. from the residual branch
        ga = torch.randn(2, C, H, H, dtype=torch.float64)
        (gc_ref,) = torch.autograd.grad([yp, y], c, [gy, ga])
        gab = buf_from(ga, 0, "constant")
    else:
        (gc_ref,) = torch.autograd.grad(yp, c, gy)
        gab = None
    cb = buf_from(c.detach(), 0, "constant")
    rb = buf_from(r, 0, "constant") if residual else None
    mean, rstd = ops.in_stats(cb)
    pad = max(fold, 1)
    out = Buf.empty(2, H, H, C, pad, DEV)
    ops.in_apply(cb, mean, rstd, act, rb, out, 1 if fold else 0)
    assert nrel(out.nhwc().permute(0, 3, 1, 2).cpu(), yp) < KTOL
    # backward: gradient of the padded output -> fold when reflect, else interior only
    gdst = Buf.empty(2, H, H, C, 2, DEV)
    bias_g = torch.empty(C, device=DEV)
    if fold:
        gsrc = buf_from(gy, 0, "constant")
        gsrc = Buf(gsrc.t, 2, H + 2 * fold, H + 2 * fold, C, 0)
        ops.in_bwd(gsrc, fold, gab, cb, mean, rstd, act, gdst, bias_g)
    else:
        gsrc = buf_from(gy[:, :, pad:-pad, pad:-pad], 0, "constant")
        ops.in_bwd(gsrc, 0, gab, cb, mean, rstd, act, gdst, bias_g)
    torch.cuda.synchronize()
    assert nrel(nchw(gdst), gc_ref) < 1e-5
    assert float(gdst.nhwc()[:, 0].abs().max()) == 0.0       # zero border
    assert abs(float(bias_g.sum())) < 1e-3


@pytest.mark.parametrize("act,fold,residual,C,gadd,gsum,H,W", [
    (1, 1, False, 256, True, True, 24, 20), (1, 1, False, 256, False, False, 17, 23),
    (0, 0, True, 256, True, False, 16, 16), (2, 0, False, 64, False, False, 33, 9),
    (1, 3, False, 32, True, True, 12, 15), (2, 1, False, 16, True, False, 11, 11),
    (1, 1, True, 512, False, False, 8, 8), (0, 0, True, 128, True, False, 10, 14)])
def test_instnorm_row_forms_bit_identical(act, fold, residual, C, gadd, gsum, H, W):
    """The row / load-batched forms of the norm passes (fg_set_in_rows 1, the default) give bit-identical
    outputs, gathered gradients, bias gradients and absmax slots to the grid-stride forms (0): ragged widths,
    fold 0 / 1 / 3, residual, gadd, gsum, C = 16 ... 512"""
    from floodgan import _lib as L, ops
    from floodgan.plans import Buf
    lib = L.load()
    torch.manual_seed(11)
    c = torch.randn(2, C, H, W, dtype=torch.float64) * 2 + 0.7
    cb = buf_from(c, 0, "constant")
    rb = buf_from(torch.randn(2, C, H, W, dtype=torch.float64), 0, "constant") if residual else None
    gsrc = Buf(buf_from(torch.randn(2, C, H + 2 * fold, W + 2 * fold, dtype=torch.float64), 0, "constant").t,
               2, H + 2 * fold, W + 2 * fold, C, 0)
    gab = buf_from(torch.randn(2, C, H, W, dtype=torch.float64), 0, "constant") if gadd else None
    mean, rstd = ops.in_stats(cb)
    outs = []
    try:
        for rows in (0, 1):
            assert lib.fg_set_in_rows(rows) == 0
            pad = max(fold, 1)
            out = Buf.empty(2, H, W, C, pad, DEV)
            out.t.fill_(7.0)
            ops.in_apply(cb, mean, rstd, act, rb, out, 1 if fold else 0)
            gdst = Buf.empty(2, H, W, C, 1, DEV)
            gdst.t.fill_(7.0)
            gs = Buf.empty(2, H, W, C, 0, DEV) if gsum else None
            bias_g = torch.full((C,), 3.0, device=DEV)
            ops.in_bwd(gsrc, fold, gab, cb, mean, rstd, act, gdst, bias_g, bias_accumulate=True, gsum=gs)
            torch.cuda.synchronize()
            # absmax slots: sharded by workgroup, so only their max is compared
            outs.append([out.t.clone(), ops.slot_of(out).max().clone(), gdst.t.clone(),
                         ops.slot_of(gdst).max().clone(), bias_g.clone()] + ([gs.t.clone()] if gsum else []))
    finally:
        lib.fg_set_in_rows(1)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


FUSED_CASES = [("resblock 3x3 s1 256->256", 256, 256, 3, 1, 1, 32, False, 0.0),
               ("resblock, large mean", 256, 256, 3, 1, 1, 32, False, 40.0),
               ("conv2 3x3 s2 64->128", 64, 128, 3, 2, 1, 64, False, 0.0),
               ("disc 4x4 s2 128->256", 128, 256, 4, 2, 1, 64, False, 0.0),
               ("deconv1 convT 256->128 (4 phases)", 256, 128, 3, 2, 1, 16, True, 0.0),
               ("deconv2 convT 128->64 (4 phases)", 128, 64, 3, 2, 1, 32, True, 0.0)]


@pytest.mark.parametrize("conv_math", ["f16x3"], indirect=True)
@pytest.mark.parametrize("case", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_fused_in_stats(case, conv_math):
    """InstanceNorm statistics from the pipelined conv kernel's epilogue (per-32-row (mean, M2) partials
    merged in fp64) agree with the standalone fg_in_stats pass over the same conv output within 1e-5, and
    the epilogue leaves the conv output bit-identical"""
    from floodgan import ops, plans as PL
    from floodgan.plans import Buf
    _, ci, co, k, s, p, H, transposed, shift = case
    torch.manual_seed(11)
    N = 2
    x = torch.randn(N, ci, H, H)
    X = buf_from(x, p if not transposed else 1, "reflect" if (k == 3 and s == 1) else "constant")
    if transposed:
        w = torch.randn(ci, co, k, k) * 0.05
        maps = PL.phase_maps(w.shape, 3, 1, ci)
        wps = [ops.pack_weight(w.to(DEV), m) for m, _, _ in maps]
        Ho = 2 * H
        mk = lambda Y: PL.phase_problems(X, w.shape, 3, 1, Y, wps, maps, bias=b)  # noqa: E731
    else:
        w = torch.randn(co, ci, k, k) * 0.05
        m = PL.wmap_conv_fwd(w.shape, ci)
        wp = ops.pack_weight(w.to(DEV), m)
        Ho = PL.out_size(H, k, s, p)
        mk = lambda Y: [PL.conv_problem(X, p, k, s, wp, m, Y, bias=b)]  # noqa: E731
    b = (torch.randn(co) * 0.1 + shift).to(DEV)
    Y0 = Buf.empty(N, Ho, Ho, co, 0, DEV)
    assert ops.conv(mk(Y0)) is None
    Y1 = Buf.empty(N, Ho, Ho, co, 0, DEV)
    st = ops.conv(mk(Y1), in_stats=True)
    assert st is not None, "the pipelined kernel should take this conv with epilogue statistics"
    mean_ref, rstd_ref = ops.in_stats(Y1)
    torch.cuda.synchronize()
    assert torch.equal(Y0.interior(), Y1.interior())
    assert nrel(st[0], mean_ref) < KTOL
    assert nrel(st[1], rstd_ref) < KTOL
    # and against fp64 statistics of the output itself
    y = Y1.interior().double().cpu()
    mu = y.mean(dim=(1, 2))
    var = y.var(dim=(1, 2), unbiased=False)
    assert nrel(st[0].view(N, co), mu) < KTOL
    assert nrel(st[1].view(N, co), (var + 1e-5).rsqrt()) < KTOL


def _decode_presplit(B, slot):
    """values of a FG_PRESPLIT buffer (include/floodgan.h): per 8 channels h[8] | l[8] of v * s, s the pow2
    scale of the slot's max (pow2_of in amax_slot.hpp)"""
    import math
    e = math.frexp(float(slot.max()))[1]
    s = 2.0 ** (14 - e)
    hl = B.t.view(torch.float16).view(-1, 2, 8).double()
    return ((hl[:, 0] + hl[:, 1]) / s).reshape(-1), s


@pytest.mark.parametrize("act,fold,C,H,W,gadd", [(1, 1, 256, 16, 20, True), (0, 1, 256, 12, 12, False),
                                                 (1, 0, 64, 9, 13, False), (0, 0, 128, 8, 8, True)])
def test_presplit_norm_outputs(act, fold, C, H, W, gadd):
    """fg_in_apply_presplit / fg_in_bwd_presplit: the FG_PRESPLIT pieces decode to the fp32 passes' outputs within
    the pieces' 22-bit precision (plus the fp16 subnormal floor at the scale), and the published scale slot bounds
    the output (the f16x3 convs derive their scale from it)"""
    from floodgan import ops
    from floodgan.plans import Buf
    torch.manual_seed(5)
    c = torch.randn(2, C, H, W, dtype=torch.float64) * 1.5 + 0.3
    cb = buf_from(c, 0, "constant")
    mean, rstd = ops.in_stats(cb)
    pad = max(fold, 1)
    ref = Buf.empty(2, H, W, C, pad, DEV)
    ops.in_apply(cb, mean, rstd, act, None, ref, 1 if fold else 0)
    ps = Buf.empty(2, H, W, C, pad, DEV)
    ops.in_apply(cb, mean, rstd, act, None, ps, 1 if fold else 0, presplit=True)
    assert ops.is_presplit(ps) and not ops.is_presplit(ref)
    torch.cuda.synchronize()
    dec, s = _decode_presplit(ps, ops.slot_of(ps))
    r = ref.t.double()
    assert float(ops.slot_of(ps).max()) >= float(r.abs().max())
    assert bool(((dec - r).abs() <= 2.0 ** -21 * r.abs() + 4 * 2.0 ** -24 / s).all())
    # backward (fold / gadd / gsum as the resblock uses them)
    gsrc = Buf(buf_from(torch.randn(2, C, H + 2 * fold, W + 2 * fold, dtype=torch.float64), 0, "constant").t,
               2, H + 2 * fold, W + 2 * fold, C, 0)
    gab = buf_from(torch.randn(2, C, H, W, dtype=torch.float64), 0, "constant") if gadd else None
    outs = []
    for presplit in (False, True):
        g = Buf.empty(2, H, W, C, 2, DEV)
        gs = Buf.empty(2, H, W, C, 0, DEV) if gadd else None
        bias_g = torch.zeros(C, device=DEV)
        ops.in_bwd(gsrc, fold, gab, cb, mean, rstd, act, g, bias_g, gsum=gs, presplit=presplit)
        outs.append((g, gs, bias_g))
    torch.cuda.synchronize()
    (gr, gsr, br), (gp, gsp, bp) = outs
    dec, s = _decode_presplit(gp, ops.slot_of(gp))
    r = gr.t.double()
    assert float(ops.slot_of(gp).max()) >= float(r.abs().max())
    assert bool(((dec - r).abs() <= 2.0 ** -21 * r.abs() + 4 * 2.0 ** -24 / s).all())
    assert torch.equal(br, bp)
    if gadd:
        assert torch.equal(gsr.t, gsp.t)


@pytest.mark.parametrize("act,residual,pad_mode", [(0, True, 1), (0, True, 0), (1, False, 1)])
def test_in_apply_dual(act, residual, pad_mode):
    """fg_in_apply_dual: the fp32 output equals fg_in_apply's bit for bit (absmax slot included), and the pre-split copy
    decodes to it within the pieces' precision, its published bound (sqrt(HW-1) + max|residual|) covering it"""
    from floodgan import ops
    from floodgan.plans import Buf
    torch.manual_seed(23)
    N, H, W, C = 2, 12, 10, 256
    c = torch.randn(N, C, H, W, dtype=torch.float64) * 2 + 0.5
    cb = buf_from(c, 0, "constant")
    rb = buf_from(torch.randn(N, C, H, W, dtype=torch.float64) * 3, 0, "constant") if residual else None
    mean, rstd = ops.in_stats(cb)
    ref = Buf.empty(N, H, W, C, 1, DEV)
    ops.in_apply(cb, mean, rstd, act, rb, ref, pad_mode)
    out, ps = Buf.empty(N, H, W, C, 1, DEV), Buf.empty(N, H, W, C, 1, DEV)
    ops.in_apply(cb, mean, rstd, act, rb, out, pad_mode, ps_copy=ps)
    torch.cuda.synchronize()
    assert torch.equal(out.t, ref.t) and float(ops.slot_of(out).max()) == float(ops.slot_of(ref).max())
    assert ops.is_presplit(ps) and not ops.is_presplit(out)
    dec, s = _decode_presplit(ps, ops.slot_of(ps))
    r = ref.t.double()
    assert float(ops.slot_of(ps).max()) >= float(r.abs().max())
    assert bool(((dec - r).abs() <= 2.0 ** -21 * r.abs() + 4 * 2.0 ** -24 / s).all())


@pytest.mark.parametrize("N,H", [(2, 16), (1, 24)])
def test_presplit_resblock_convs(N, H):
    """The resblock convs on FG_PRESPLIT operands (the pipelined forward, its input-gradient interior + edge strips,
    the pipelined weight gradient with pre-split gradient and / or activation) vs fp64, and vs the same convs on the
    fp32 buffers"""
    from floodgan import executor as X, ops, plans as PL
    from floodgan.plans import Buf
    C = 256
    torch.manual_seed(7)
    c = torch.randn(N, C, H, H, dtype=torch.float64)
    w = torch.randn(C, C, 3, 3, dtype=torch.float64) * 0.03
    P = {"conv.weight": w.float().to(DEV), "conv.bias": torch.zeros(C, device=DEV)}
    cb = buf_from(c, 0, "constant")
    mean, rstd = ops.in_stats(cb)
    xs = {}
    for presplit in (False, True):
        xb = Buf.empty(N, H, H, C, 1, DEV)
        ops.in_apply(cb, mean, rstd, 1, None, xb, 1, presplit=presplit)
        xs[presplit] = xb
    x64 = F.relu(F.instance_norm(c, eps=1e-5))
    y64 = F.conv2d(F.pad(x64, (1,) * 4, mode="reflect"), w)
    gy64 = torch.randn_like(y64)
    # gradient operand: the fp32 / pre-split outputs of one norm backward (act none, no fold)
    gsrc = buf_from(gy64, 0, "constant")
    gys = {}
    for presplit in (False, True):
        g = Buf.empty(N, H, H, C, 2, DEV)
        ops.in_bwd(gsrc, 0, None, cb, mean, rstd, 0, g, None, presplit=presplit)
        gys[presplit] = g
    gref = nchw(gys[False]).double()
    gx64, gw64 = torch.autograd.grad(F.conv2d(F.pad(x64.requires_grad_(True), (1,) * 4, mode="reflect"),
                                              w.requires_grad_(True)), (x64, w), gref)
    res = {}
    for presplit in (False, True):
        Y = Buf.empty(N, H, H, C, 0, DEV)
        X._conv_fwd(P, "conv", xs[presplit], 1, 3, 1, Y)
        dw = torch.empty(C, C, 3, 3, device=DEV)
        ops.wgrad(PL.wgrad_conv(gys[presplit], xs[presplit], 1, 3, 1, C), PL.wmap_wgrad(w.shape, True, C, 3), dw)
        dw_p = torch.empty(C, C, 3, 3, device=DEV)      # gradient pre-split, activation fp32
        ops.wgrad(PL.wgrad_conv(gys[presplit], xs[False], 1, 3, 1, C), PL.wmap_wgrad(w.shape, True, C, 3), dw_p)
        gxp = X._dgrad_s1_padded(P, "conv", gys[presplit])
        torch.cuda.synchronize()
        res[presplit] = (nchw(Y), dw.cpu(), dw_p.cpu(), _fold_cpu(nchw(gxp).double(), 1))
    for presplit in (False, True):
        y, dw, dw_p, gx = res[presplit]
        assert nrel(y, y64) < KTOL and nrel(dw, gw64) < KTOL and nrel(dw_p, gw64) < KTOL and nrel(gx, gx64) < KTOL
    for a, b in zip(res[False], res[True]):
        assert nrel(b, a) < 2e-6


@pytest.mark.parametrize("persistent", [1, 3])
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
@pytest.mark.parametrize("case", [(256, 256, 3, 1, 1, 20), (128, 64, 3, 2, 1, 24), (64, 128, 3, 1, 1, 17)])
def test_presplit_f3_tiles_and_stats(case, cfg, persistent):
    """every pipelined tile config (and the automatic choice, -1) on a FG_PRESPLIT operand, with and without the
    InstanceNorm statistics epilogue (32-row blocks of 32- and 64-row wave tiles), ragged tiles and the
    tile-crossing stream (persistent 3): output vs fp64, statistics vs fg_in_stats of the same output, output
    bit-identical with and without the epilogue statistics"""
    from floodgan import _lib as L, ops, plans as PL
    from floodgan.plans import Buf
    cin, cout, k, s, p, H = case
    lib = L.load()
    try:
        L.set_f3_tile(cfg)
        lib.fg_set_f3_persistent(persistent)
        torch.manual_seed(13)
        N = 2
        c = torch.randn(N, cin, H, H, dtype=torch.float64) * 1.3 + 0.2
        cb = buf_from(c, 0, "constant")
        mean, rstd = ops.in_stats(cb)
        X = Buf.empty(N, H, H, cin, p, DEV)
        ops.in_apply(cb, mean, rstd, 1, None, X, 1, presplit=True)
        x64 = F.relu(F.instance_norm(c, eps=1e-5))
        w = torch.randn(cout, cin, k, k, dtype=torch.float64) * 0.05
        b = torch.randn(cout, dtype=torch.float64) * 0.1
        y64 = F.conv2d(F.pad(x64, (p,) * 4, mode="reflect"), w, b, stride=s)
        wd = w.float().to(DEV)
        m = PL.wmap_conv_fwd(wd.shape, cin)
        wp = ops.pack_weight(wd, m)
        Ho = PL.out_size(H, k, s, p)
        Ys = []
        for stats in (False, True):
            Y = Buf.empty(N, Ho, Ho, cout, 0, DEV)
            st = ops.conv([PL.conv_problem(X, p, k, s, wp, m, Y, bias=b.float().to(DEV))], in_stats=stats)
            Ys.append((Y, st))
        torch.cuda.synchronize()
        (Y0, _), (Y1, st) = Ys
        assert nrel(nchw(Y0), y64) < KTOL
        assert torch.equal(Y0.interior(), Y1.interior())
        if (Ho * Ho) % 32 == 0:
            assert st is not None
            mean_ref, rstd_ref = ops.in_stats(Y1)
            assert nrel(st[0], mean_ref) < KTOL and nrel(st[1], rstd_ref) < KTOL
    finally:
        L.set_f3_tile(-1)
        lib.fg_set_f3_persistent(1)


@pytest.mark.parametrize("persistent", [1, 3])
@pytest.mark.parametrize("N,cin,H,W", [(2, 128, 16, 16), (1, 128, 9, 7), (2, 256, 12, 10), (8, 128, 64, 64)])
def test_quad_convT(N, cin, H, W, persistent):
    """The quad form (one problem for the 4 output phases of a stride-2 3-tap transposed op, zero segments
    skipped: plans.quad_map / conv_f3.hip QUAD) on a FG_PRESPLIT operand: ConvTranspose2d(cin, 64, 3, 2, 1, 1)
    with bias, and the input gradient of Conv2d(64, cin, 3, 2, 1), vs fp64; the forward's epilogue statistics vs
    fg_in_stats of its output; bit-identical outputs with and without the statistics; ragged tiles (9 x 7),
    the tile-crossing stream (persistent 3) -- and the executor routing deconv2 / conv2's input gradient to it"""
    from floodgan import _lib as L, executor as X, ops, plans as PL
    from floodgan.plans import Buf
    lib = L.load()
    try:
        lib.fg_set_f3_persistent(persistent)
        torch.manual_seed(17)
        c = torch.randn(N, cin, H, W, dtype=torch.float64) * 1.2 + 0.1
        cb = buf_from(c, 0, "constant")
        mean, rstd = ops.in_stats(cb)
        S = Buf.empty(N, H, W, cin, 1, DEV)
        ops.in_apply(cb, mean, rstd, 1, None, S, 0, presplit=True)        # relu(IN(c)), zero border, pre-split
        x64 = F.relu(F.instance_norm(c, eps=1e-5))
        w = torch.randn(cin, 64, 3, 3, dtype=torch.float64) * 0.05
        b = torch.randn(64, dtype=torch.float64) * 0.1
        y64 = F.conv_transpose2d(x64, w, b, stride=2, padding=1, output_padding=1)
        inp = torch.zeros(N, 64, 2 * H, 2 * W, dtype=torch.float64, requires_grad=True)
        g64, = torch.autograd.grad(F.conv2d(inp, w, stride=2, padding=1), inp, x64)
        P = {"t.weight": w.float().to(DEV), "t.bias": b.float().to(DEV)}
        assert X._quad_ok(S, w.shape, 3, Buf.empty(N, 2 * H, 2 * W, 64, 0, DEV))
        outs = []
        for stats in (False, True):
            Y = Buf.empty(N, 2 * H, 2 * W, 64, 0, DEV)
            st = X._quad(P, "t", S, Y, bias=P["t.bias"], in_stats=stats)
            assert ops.LAST_CONV_KERNEL == "conv_fwd_f3_quad"
            outs.append((Y, st))
        G = Buf.empty(N, 2 * H, 2 * W, 64, 0, DEV)
        X._dgrad_s2(P, "t", S, 3, Y=G)
        assert ops.LAST_CONV_KERNEL == "conv_fwd_f3_quad"
        Yr = Buf.empty(N, 2 * H, 2 * W, 64, 0, DEV)
        st_r = X._convT_fwd(P, "t", S, Yr)
        torch.cuda.synchronize()
        (Y0, _), (Y1, st) = outs
        assert nrel(nchw(Y0), y64) < KTOL, nrel(nchw(Y0), y64)
        assert torch.equal(Y0.interior(), Y1.interior()) and torch.equal(Yr.interior(), Y0.interior())
        assert nrel(nchw(G), g64) < KTOL, nrel(nchw(G), g64)
        if (H * W) % 32 == 0:
            assert st is not None and st_r is not None
            mean_ref, rstd_ref = ops.in_stats(Y1)
            assert nrel(st[0], mean_ref) < KTOL and nrel(st[1], rstd_ref) < KTOL
    finally:
        lib.fg_set_f3_persistent(1)


def test_fused_in_stats_declined():
    """a conv the epilogue statistics cannot cover (output rows per image not a multiple of 32, e.g. the
    discriminator's 4x4 stride-1 conv) returns None and the caller computes the statistics itself"""
    from floodgan import ops, plans as PL
    from floodgan.plans import Buf
    torch.manual_seed(12)
    X = buf_from(torch.randn(2, 256, 16, 16), 1, "constant")
    w = torch.randn(512, 256, 4, 4, device=DEV) * 0.05
    m = PL.wmap_conv_fwd(w.shape, 256)
    Y = Buf.empty(2, 15, 15, 512, 0, DEV)
    assert ops.conv([PL.conv_problem(X, 1, 4, 1, ops.pack_weight(w, m), m, Y)], in_stats=True) is None


# ------------------------------------------------------------------ tail, losses, adam

@pytest.mark.parametrize("H,W", [(16, 16), (19, 300)])
def test_tail(H, W):
    """Generator tail forward / backward; (19, 300): the 256-pixel blocks of the LDS-staged kernels
    straddle rows, images and g_content's zero border."""
    from floodgan import ops
    from floodgan.plans import Buf
    torch.manual_seed(4)
    N = 2
    cl = torch.randn(N, 27, H, W, dtype=torch.float64, requires_grad=True)
    al = torch.randn(N, 10, H, W, dtype=torch.float64, requires_grad=True)
    x = torch.randn(N, 9, H, W, dtype=torch.float64)
    t = torch.tanh(cl)
    a = torch.softmax(al, 1)
    out = sum(t[:, 3 * i:3 * i + 3] * a[:, i:i + 1] for i in range(9)) + x[:, :3] * a[:, 9:10]
    g = torch.randn_like(out)
    gcl_ref, gal_ref = torch.autograd.grad(out, (cl, al), g, retain_graph=True)
    CL = buf_from(cl.detach(), 0, "constant", 32)
    AL = buf_from(al.detach(), 0, "constant", 16)
    xd = x.float().to(DEV)
    o = torch.empty(N, 3, H, W, device=DEV)
    mk = torch.empty(N, H, W, device=DEV)
    ops.tail_fwd(CL, AL, xd, o, mk)
    assert nrel(o, out) < KTOL and nrel(mk, a[:, 9]) < KTOL
    GC = Buf.empty(N, H, W, 32, 6, DEV)
    GA = Buf.empty(N, H, W, 16, 0, DEV)
    GC.t.fill_(float("nan"))
    GA.t.fill_(float("nan"))
    ops.tail_bwd(CL, AL, xd, g.float().to(DEV), GC, GA)
    torch.cuda.synchronize()
    assert nrel(nchw(GC, 27), gcl_ref) < KTOL and nrel(nchw(GA, 10), gal_ref) < KTOL
    assert float(GC.nhwc()[..., 27:].abs().max()) == 0.0 and float(GC.nhwc()[:, :6].abs().max()) == 0.0
    # the kernel raised both outputs' absmax slots (the f16x3 scale sources of the convs reading them)
    from floodgan import _lib as L
    if L.fwd_f16x3():
        assert float(ops.slot_of(GC).max()) == float(GC.t.abs().max())
        assert float(ops.slot_of(GA).max()) == float(GA.t.abs().max())
        assert ops.absmax(GC) is ops.slot_of(GC)          # cached: no separate pass
    # a loss on last_attention_mask (attention10) as well: its gradient joins attention channel 9's
    gm = torch.randn(N, H, W, dtype=torch.float64)
    gcl_ref2, gal_ref2 = torch.autograd.grad((out, a[:, 9]), (cl, al), (g, gm))
    gm_d = gm.float().to(DEV).permute(1, 2, 0).contiguous().permute(2, 0, 1)     # a strided [N, H, W] view
    ops.tail_bwd(CL, AL, xd, g.float().to(DEV), GC, GA, g_mask=gm_d)
    torch.cuda.synchronize()
    assert nrel(nchw(GC, 27), gcl_ref2) < KTOL and nrel(nchw(GA, 10), gal_ref2) < KTOL


def test_losses_and_adam():
    from floodgan import ops
    torch.manual_seed(5)
    p = torch.randn(2, 1, 62, 62)
    loss = torch.empty(1, device=DEV)
    g = torch.empty(2, 1, 62, 62, device=DEV)
    ops.mse_const(p.to(DEV), 1.0, 0.5, loss, g)
    pr = p.double().requires_grad_(True)
    ref = F.mse_loss(pr, torch.ones_like(pr))
    (gr,) = torch.autograd.grad(ref * 0.5, pr)
    assert abs(float(loss) - float(ref)) < 1e-6 * float(ref) + 1e-7 and nrel(g, gr) < 1e-6
    a = torch.randn(2, 3, 16, 16)
    b = torch.randn(2, 3, 16, 16)
    gl = torch.empty(2, 3, 16, 16, device=DEV)
    ops.l1(a.to(DEV), b.to(DEV), 100.0, loss, gl)
    ar = a.double().requires_grad_(True)
    ref = F.l1_loss(ar, b.double())
    (gr,) = torch.autograd.grad(ref * 100, ar)
    assert abs(float(loss) - float(ref)) < 1e-6 and nrel(gl, gr) < 1e-6
    l1v = float(loss)
    ops.l1(a.to(DEV), b.to(DEV), 100.0, loss, gl, loss_scale=100.0)      # the logged 100 * L1, scaled in fp32
    assert float(loss) == float(torch.tensor(l1v, dtype=torch.float32) * 100.0)
    # Adam against torch.optim.Adam on the CPU (the oracle's optimiser), 3 steps
    from floodgan.optim import FusedAdam
    w0 = torch.randn(1000) * 0.02
    pc = torch.nn.Parameter(w0.clone())
    pd = torch.nn.Parameter(w0.clone().to(DEV))
    oc = torch.optim.Adam([pc], lr=2e-4, betas=(0.5, 0.999))
    od = FusedAdam([pd], lr=2e-4, betas=(0.5, 0.999))
    for _ in range(3):
        gg = torch.randn(1000)
        pc.grad = gg.clone()
        pd.grad = gg.clone().to(DEV)
        oc.step()
        od.step()
    torch.cuda.synchronize()
    assert float((pd.detach().cpu() - pc.detach()).abs().max()) < 1e-9 + 1e-6 * float(pc.detach().abs().max())
    sd_c, sd_d = oc.state_dict(), od.state_dict()
    assert sd_c["param_groups"][0].keys() == sd_d["param_groups"][0].keys()
    assert float(sd_d["state"][0]["step"]) == 3.0


@pytest.mark.parametrize("conv_math", ["f16x3"], indirect=True)
def test_pack_cache_and_batched_repack(conv_math):
    """The f16x3 pack cache: a parameter's packed layouts are reused while current, re-packed by
    FusedAdam's step in batched launches (fg_pack_weight_f16_batch, > FG_PACK_BATCH_MAX jobs here), and
    every cached pack is bit-identical to a fresh fg_pack_weight_f16 of the current values; a torch
    in-place write makes the next pack_weight pack afresh"""
    from floodgan import _lib as L, ops, plans as PL
    from floodgan.optim import FusedAdam
    torch.manual_seed(21)
    params, maps = [], []
    for i in range(9):      # 9 parameters x 3-6 layouts each = 36 cached packs
        w = torch.nn.Parameter((torch.randn(64, 32 + 16 * (i % 3), 3, 3) * 0.05).to(DEV))
        ms = [PL.wmap_conv_fwd(w.shape, w.shape[1]), PL.wmap_conv_dgrad_s1(w.shape, w.shape[0])]
        ms += [m for m, _, _ in PL.phase_maps(w.shape, 3, 1, w.shape[0])][:1 + i % 4]
        params.append(w)
        maps.append(ms)
    packs = [[ops.pack_weight(w, m) for m in ms] for w, ms in zip(params, maps)]
    assert sum(len(p) for p in packs) > L.FG_PACK_BATCH_MAX
    # current: the same tensors come back
    assert all(ops.pack_weight(w, m) is wp for w, ms, ps in zip(params, maps, packs) for m, wp in zip(ms, ps))
    opt = FusedAdam(params, lr=1e-2, betas=(0.5, 0.999))
    for _ in range(2):
        for w in params:
            w.grad = torch.randn_like(w)
        opt.step()
        for w, ms, ps in zip(params, maps, packs):
            for m, wp in zip(ms, ps):
                assert ops.pack_weight(w, m) is wp            # re-packed in place by the step
                s = ops.wmap_struct(m)
                ref = torch.empty_like(wp)
                L.check(L.load().fg_pack_weight_f16(L.ptr(w), C.byref(s), L.ptr(ops.pack_slot(wp)), L.ptr(ref),
                                                    L.stream_handle()), "pack")
                torch.cuda.synchronize()
                assert torch.equal(ref.view(torch.int16), wp.view(torch.int16))
    # a torch write: the cached pack is stale and pack_weight packs the new values
    w, m, wp = params[0], maps[0][0], packs[0][0]
    with torch.no_grad():
        w.mul_(3.0)
    wp2 = ops.pack_weight(w, m)
    assert wp2 is not wp
    s = ops.wmap_struct(m)
    ref = torch.empty_like(wp2)
    L.check(L.load().fg_pack_weight_f16(L.ptr(w), C.byref(s), L.ptr(ops.pack_slot(wp2)), L.ptr(ref),
                                        L.stream_handle()), "pack")
    torch.cuda.synchronize()
    assert torch.equal(ref.view(torch.int16), wp2.view(torch.int16))


# ------------------------------------------------------------------ modules / step
#
# Parity criteria:
#  P1  everything computed BEFORE the first optimiser update -- G output, attention mask, D
#      outputs, the D losses and the L1 term -- within 1e-5 of the reference's own fp32 run
#      (golden vectors) or the fp64 oracle.
#  P2  gradients through the whole G+D graph under a smooth loss within 1e-4 of fp64, at a size
#      where no ReLU kink sits within fp32 rounding of zero (32x32; scripts/diag_mask.py counts
#      the flips: 0 at 32x32, 1 at 64x64, and that single flipped mask element moves every
#      upstream gradient by ~3e-3 -- in the reference's own fp32-vs-fp64 comparison too).
#  P3  state AFTER Adam updates: within 2x the reference's own sensitivity envelope -- the largest
#      deviation of the reference algorithm (CPU oracle, fp32) from its unperturbed run when its
#      inputs carry 1e-6 relative noise (the size of an fp32 forward's rounding), 4 trials -- and
#      never worse than that envelope + the north-star 1e-3 where the envelope is below it.
#      Adam's first steps are sign-like (m/sqrt(v) = +-1) and ReLU / L1 kinks flip, so after an
#      update no fp32 implementation can track the reference to 1e-3: the reference itself moves
#      by 1.5e-3 (32x32) and 1.7e-2 (64x64) under such noise (tests/test_oracle_sensitivity.py).


def _make_model():
    from floodgan.model import Model
    return Model(model="PairedAttention", num_epochs=2, topography="all")


def _worst(pairs):
    w = max(pairs, key=lambda t: t[1])
    return w[0], w[1]


@pytest.mark.parametrize("R", [32, 64])
def test_modules_forward_vs_golden(golden, R, report):
    """P1: forward of the drop-in modules at the seed-47 initialisation vs the reference."""
    g = golden(R)
    m = _make_model()
    x0 = torch.from_numpy(g["x0"]).to(DEV)
    y0 = torch.from_numpy(g["y0"]).to(DEV)
    with torch.no_grad():
        out = m.generator(x0)
        mask = m.generator.last_attention_mask
        d = m.discriminator(torch.cat((x0, y0), 1))
    e = dict(g_out=nrel(out, torch.from_numpy(g["init_g_out"])), mask=nrel(mask, torch.from_numpy(g["init_mask"])),
             d_out=nrel(d, torch.from_numpy(g["init_d_out"])))
    report("forward_vs_reference_golden", R=R, **e)
    assert max(e.values()) < 1e-5, e


def test_module_autograd_vs_fp64(report):
    """P2: gradients of G and D through the drop-in modules (torch autograd over the two fused
    nodes) vs the fp64 oracle, smooth loss MSE(D(cat(x, G(x))), 1) + 100*MSE(G(x), y).  The oracle's
    ReLU / LeakyReLU decisions are teacher-forced to the HIP path's (read from a deterministic re-run of
    the same forward through the executor): at 32x32 one decision flipped by rounding moves a weight
    gradient by ~1e-4; every differing decision must sit within rounding of its kink."""
    from floodgan import executor as X
    R = 32
    torch.manual_seed(11)
    x = torch.rand(2, 9, R, R) * 2 - 1
    y = torch.rand(2, 3, R, R) * 2 - 1
    m = _make_model()
    xd, yd = x.to(DEV), y.to(DEV)
    fake = m.generator(xd)
    pred = m.discriminator(torch.cat((xd, fake), 1))
    (F.mse_loss(pred, torch.ones_like(pred)) + 100 * F.mse_loss(fake, yd)).backward()
    with torch.no_grad():
        fake_s, _, S = X.gen_forward(m.generator.param_dict(), xd, save=True)
        _, dS = X.disc_forward(m.discriminator.param_dict(), X.disc_pack([(xd, fake_s)], 12), save=True)
        dec = O.ActDecisions({"G": [X.gen_act_decisions(S)], "D": [X.disc_act_decisions(dS)]})
    torch.cuda.synchronize()
    Gp, Dp = O.init_params()
    Gd = {k: v.double().requires_grad_(True) for k, v in Gp.items()}
    Dd = {k: v.double().requires_grad_(True) for k, v in Dp.items()}
    fake_r, _ = O.generator_forward(Gd, x.double(), O._forced(dec, "G"))
    pr = O.discriminator_forward(Dd, torch.cat((x.double(), fake_r), 1), O._forced(dec, "D"))
    (F.mse_loss(pr, torch.ones_like(pr)) + 100 * F.mse_loss(fake_r, y.double())).backward()
    skip_g, skip_d = O.cancelled_biases()
    eg = [(k, nrel(p.grad, Gd[k].grad)) for k, p in m.generator.named_parameters() if k not in skip_g]
    ed = [(k, nrel(p.grad, Dd[k].grad)) for k, p in m.discriminator.named_parameters() if k not in skip_d]
    flips = sum(n for _, _, n, _ in dec.log)
    report("grad_vs_fp64_smooth_loss", R=R, worst_G=_worst(eg), worst_D=_worst(ed), decisions_differing=flips,
           worst_kink=dec.worst())
    assert _worst(eg)[1] < 1e-4 and _worst(ed)[1] < 1e-4, (_worst(eg), _worst(ed))
    assert dec.worst() < 1e-4, dec.worst()


def _reference_envelope(g, sigma=1e-6, trials=4):
    """P3 envelope: max deviation (G out, D out, losses) of the reference algorithm (CPU oracle,
    fp32) from the golden run when its inputs carry `sigma` relative noise."""
    x0, y0 = torch.from_numpy(g["x0"]), torch.from_numpy(g["y0"])
    env = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    for trial in range(1, trials + 1):
        torch.manual_seed(trial)
        st = O.PairedStepOracle()
        for it in range(2):
            st.set_lr(float(g[f"it{it}_lr"][0]))
            x, y = torch.from_numpy(g[f"x{it}"]), torch.from_numpy(g[f"y{it}"])
            ls = np.array(st.step(x * (1 + sigma * torch.randn_like(x)), y))
            with torch.no_grad():
                go, _ = O.generator_forward(st.G, x0)
                do = O.discriminator_forward(st.D, torch.cat((x0, y0), 1))
            e = (nrel(go, torch.from_numpy(g[f"it{it}_g_out"])), nrel(do, torch.from_numpy(g[f"it{it}_d_out"])),
                 float((np.abs(ls - g[f"it{it}_losses"]) / np.abs(g[f"it{it}_losses"])).max()))
            env[it] = [max(a, b) for a, b in zip(env[it], e)]
    return env


@pytest.mark.parametrize("R", [32, 64])
def test_paired_step_vs_golden(golden, R, report):
    """Two iterations of the fused step vs the REFERENCE's own train_paired (golden)."""
    g = golden(R)
    env = _reference_envelope(g)
    m = _make_model()
    x0 = torch.from_numpy(g["x0"]).to(DEV)
    y0 = torch.from_numpy(g["y0"]).to(DEV)
    for it in range(2):
        for opt in (m.optimizer_generator, m.optimizer_discriminator):
            for grp in opt.param_groups:
                grp["lr"] = float(g[f"it{it}_lr"][0])
        x = torch.from_numpy(g[f"x{it}"]).to(DEV)
        y = torch.from_numpy(g[f"y{it}"]).to(DEV)
        losses = m.step_fn(x, y).cpu().numpy().astype(np.float64)
        ref = g[f"it{it}_losses"].copy()
        ref[3] *= 100
        lrel = np.abs(losses - ref) / np.abs(ref)
        with torch.no_grad():
            out = m.generator(x0)
            d = m.discriminator(torch.cat((x0, y0), 1))
        e_g, e_d = nrel(out, torch.from_numpy(g[f"it{it}_g_out"])), nrel(d, torch.from_numpy(g[f"it{it}_d_out"]))
        report("step_vs_reference_golden", R=R, it=it, loss_rel=lrel.tolist(), g_out_after=e_g, d_out_after=e_d,
               reference_envelope=env[it])
        if it == 0:   # P1: the D losses and the L1 term are evaluated before any update
            assert lrel[[0, 1, 3]].max() < 1e-5, lrel
        # P3
        assert lrel.max() < max(NTOL, 2 * env[it][2]), (lrel, env[it])
        assert e_g < max(NTOL, 2 * env[it][0]), (e_g, env[it])
        assert e_d < max(NTOL, 2 * env[it][1]), (e_d, env[it])


def test_paired_step_256_vs_oracle(report):
    """Fused step at 256x256, batch 2, vs the CPU oracle in fp32 and fp64 (seed-47 weights)."""
    torch.manual_seed(7)
    R = 256
    x = torch.rand(2, 9, R, R) * 2 - 1
    y = torch.rand(2, 3, R, R) * 2 - 1
    r32, r64 = {}, {}
    s32 = O.PairedStepOracle()
    l32 = np.array(s32.step(x, y, record=r32))
    s64 = O.PairedStepOracle(dtype=torch.float64)
    l64 = np.array(s64.step(x, y, record=r64))
    torch.manual_seed(1)
    sp = O.PairedStepOracle()          # the reference under 1e-6 input noise (P3 envelope)
    sp.step(x * (1 + 1e-6 * torch.randn_like(x)), y)
    m = _make_model()
    losses = m.step_fn(x.to(DEV), y.to(DEV)).cpu().numpy().astype(np.float64)
    l32[3] *= 100
    l64[3] *= 100
    skip_g, skip_d = O.cancelled_biases()
    fake_err = nrel(m.step_fn.last_output, r64["fake"])
    fake_err32 = nrel(r32["fake"], r64["fake"])
    pg = [(k, nrel(p, s32.G[k])) for k, p in m.generator.named_parameters() if k not in skip_g]
    pg_env = [(k, nrel(sp.G[k], s32.G[k])) for k in s32.G if k not in skip_g]
    pd = [(k, nrel(p, s32.D[k])) for k, p in m.discriminator.named_parameters() if k not in skip_d]
    pd_env = [(k, nrel(sp.D[k], s32.D[k])) for k in s32.D if k not in skip_d]
    gg = [(k, nrel(p.grad, r64["g_grads"][k])) for k, p in m.generator.named_parameters() if k not in skip_g]
    gg32 = [(k, nrel(r32["g_grads"][k], r64["g_grads"][k])) for k in r32["g_grads"] if k not in skip_g]
    report("step256_vs_oracle", loss_rel_fp64=(np.abs(losses - l64) / np.abs(l64)).tolist(),
           ref32_loss_rel_fp64=(np.abs(l32 - l64) / np.abs(l64)).tolist(), fake_vs_fp64=fake_err,
           ref32_fake_vs_fp64=fake_err32, params_G_vs_ref32=_worst(pg), params_G_envelope=_worst(pg_env),
           params_D_vs_ref32=_worst(pd), params_D_envelope=_worst(pd_env), grads_G_l1_vs_fp64=_worst(gg),
           ref32_grads_G_l1_vs_fp64=_worst(gg32))
    assert fake_err < 1e-5                                                      # P1
    assert (np.abs(losses - l64) / np.abs(l64))[[0, 1, 3]].max() < 1e-5         # P1
    assert _worst(pg)[1] < max(NTOL, 2 * _worst(pg_env)[1])                     # P3
    assert _worst(pd)[1] < max(NTOL, 2 * _worst(pd_env)[1])                     # P3


def test_block_module():
    from floodgan.model_architectures import PairedAttentionBlock
    torch.manual_seed(8)
    blk = PairedAttentionBlock(256, 3, 1, 1)
    x = torch.randn(2, 256, 12, 12)
    P = {"resnet_blocks.0.conv1.weight": blk.conv1.weight.detach().double().requires_grad_(True),
         "resnet_blocks.0.conv1.bias": blk.conv1.bias.detach().double().requires_grad_(True),
         "resnet_blocks.0.conv2.weight": blk.conv2.weight.detach().double().requires_grad_(True),
         "resnet_blocks.0.conv2.bias": blk.conv2.bias.detach().double().requires_grad_(True)}
    xr = x.double().requires_grad_(True)
    yr = O.resnet_block(P, 0, xr)
    g = torch.randn_like(yr)
    yr.backward(g)
    blk = blk.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    yd = blk(xd)
    yd.backward(g.float().to(DEV))
    assert nrel(yd, yr) < 1e-5
    assert nrel(xd.grad, xr.grad) < 1e-5
    assert nrel(blk.conv1.weight.grad, P["resnet_blocks.0.conv1.weight"].grad) < 1e-5


def test_reference_loop_with_dropin_modules(golden):
    """The reference's own loop body (models/model.py:615-646: torch.cat, nn.MSELoss, nn.L1Loss,
    requires_grad toggling, two D calls with accumulated grads) driven through the drop-in
    modules + FusedAdam: one iteration vs the reference's golden at 32x32."""
    g = golden(32)
    m = _make_model()
    G, D = m.generator, m.discriminator
    og, od = m.optimizer_generator, m.optimizer_discriminator
    mse, l1 = torch.nn.MSELoss(), torch.nn.L1Loss()
    x = torch.from_numpy(g["x0"]).to(DEV)
    y = torch.from_numpy(g["y0"]).to(DEV)
    fake = G(x)
    cr, cs = torch.cat((x, y), 1), torch.cat((x, fake), 1)
    for p in D.parameters():
        p.requires_grad = True
    od.zero_grad()
    ps = D(cs.detach())
    ls = mse(ps, torch.zeros_like(ps))
    prr = D(cr)
    lr_ = mse(prr, torch.ones_like(prr))
    ((ls + lr_) * 0.5).backward()
    od.step()
    for p in D.parameters():
        p.requires_grad = False
    og.zero_grad()
    pg = D(cs)
    lg = mse(pg, torch.ones_like(pg))
    ll = l1(fake, y) * 100
    (lg + ll).backward()
    og.step()
    losses = np.array([float(lr_), float(ls), float(lg), float(ll) / 100])
    ref = g["it0_losses"]
    assert (np.abs(losses - ref) / np.abs(ref))[[0, 1, 3]].max() < 1e-5, (losses, ref)
    with torch.no_grad():
        out = G(x)
    env = _reference_envelope(g)[0][0]
    assert nrel(out, torch.from_numpy(g["it0_g_out"])) < max(NTOL, 2 * env)


# ------------------------------------------------------------------ bias-gradient sums, activation backward

@pytest.mark.parametrize("N,H,C,c_valid,pad", [(2, 33, 32, 27, 3), (2, 40, 16, 10, 0), (3, 17, 64, 64, 1),
                                               (2, 64, 4, 1, 0), (1, 9, 12, 12, 2)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_channel_sum(N, H, C, c_valid, pad, accumulate):
    """fg_channel_sum (bias gradients: models/model_architectures.py conv biases without a following
    IN) against an fp64 sum, padded views and partial channel ranges included"""
    from floodgan import ops
    torch.manual_seed(5)
    x = torch.randn(N, C, H, H, dtype=torch.float64)
    b = buf_from(x, pad, "constant")
    out = torch.randn(C, device=DEV)
    prev = out.clone()
    ops.channel_sum(b, c_valid, out, accumulate)
    torch.cuda.synchronize()
    ref = x.float().double().sum((0, 2, 3))[:c_valid] + (prev[:c_valid].double().cpu() if accumulate else 0)
    assert nrel(out[:c_valid], ref) < 1e-5
    assert torch.equal(out[c_valid:].cpu(), prev[c_valid:].cpu())


@pytest.mark.parametrize("C,act", [(64, 2), (16, 1), (3, 2)])
def test_act_bwd(C, act):
    """fg_act_bwd: g *= act'(y) over the interior of padded views (ReLU / LeakyReLU(0.2))"""
    from floodgan import ops
    torch.manual_seed(6)
    g = torch.randn(2, C, 21, 21, dtype=torch.float64)
    y = torch.randn(2, C, 21, 21, dtype=torch.float64)
    gb, yb = buf_from(g, 1, "constant"), buf_from(y, 2, "constant")
    ops.act_bwd(gb, yb, act)
    torch.cuda.synchronize()
    slope = 0.0 if act == 1 else 0.2
    ref = g.float().double() * torch.where(y.float() > 0, torch.ones_like(y), torch.full_like(y, slope))
    assert nrel(nchw(gb), ref) < 1e-6
    # border_zero: the kernel raises a fresh absmax slot of g (f16x3)
    from floodgan import _lib as L
    if L.fwd_f16x3():
        g2 = buf_from(g, 1, "constant")
        ops.act_bwd(g2, yb, act, border_zero=True)
        torch.cuda.synchronize()
        assert float(ops.slot_of(g2).max()) == float(g2.t.abs().max())


def test_pack_input_absmax_slots():
    """fg_pack_input raises dst's absmax slot: a full pack a fresh slot, a discriminator input packed in two
    parts one shared slot over both (executor.disc_pack), equal to the packed buffer's max |value|"""
    from floodgan import _lib as L, executor as X, ops
    from floodgan.plans import Buf
    if not L.fwd_f16x3():
        pytest.skip("absmax slots are kept under the f16x3 math")
    torch.manual_seed(9)
    x = (torch.randn(2, 9, 24, 24) * 3).to(DEV)
    y = (torch.randn(2, 3, 24, 24) * 7).to(DEV)
    X0 = Buf.empty(2, 24, 24, 9, 3, DEV)
    ops.pack_input(x, 9, None, 0, X0, 0, 2, 1)
    torch.cuda.synchronize()
    assert float(ops.slot_of(X0).max()) == float(X0.t.abs().max()) == float(x.abs().max())
    buf = X.disc_pack([(x, y), (x, -2 * y)], 12)
    torch.cuda.synchronize()
    assert float(ops.slot_of(buf).max()) == float(buf.t.abs().max())
    assert ops.absmax(buf) is ops.slot_of(buf)
