"""BatchNorm (training mode) kernels of csrc/bnorm.hip vs torch-CPU fp64 (nn.BatchNorm2d semantics,
models/model_architectures.py:34-35, :74-80): batch statistics per group of images (the reference's
separate D(fake) / D(real) calls fused into one pass), running statistics updated once per group in
order, the affine transform, Dropout with a given mask (x mask / 0.5), two differently activated
outputs written into a padded buffer and a channel slice of a wider one (the U-Net's cat halves), the
backward through both activations, the dropout and the group statistics; nn.MaxPool2d(2).

Every compared tensor meets both forms of the kernel bound (`close`): the norm-relative error and
max |a - b| / max |b| below KTOL -- the norm alone hides one wrong element of a large tensor.  Inputs
are fp32 values (the fp64 reference sees exactly what the kernel reads); outputs start as NaN, so an
unwritten element and a write outside the stated region both fail."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import DEV, KTOL, buf_from, nchw, nrel

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture
def f16x3():
    """the absmax slots are raised under the f16x3 conv math only"""
    from floodgan import _lib as L
    prev = L.get_conv_math()
    L.set_conv_math("f16x3")
    yield
    L.set_conv_math(prev)


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def close(what, a, b, report=None, a32=None):
    """a within KTOL of the fp64 reference b in both norms (a NaN in a fails both).  a32: the same operation in torch
    CPU float32 on the same inputs, given only for a case fp32 itself cannot hold to KTOL in the max norm: the bound
    there is 4 x the distance of a32 from b (a different summation order costs a small multiple, a wrong element
    still fails), never below KTOL"""
    e2, em = nrel(a, b), maxrel(a, b)
    bound, note = KTOL, ""
    if a32 is not None:
        spread = maxrel(a32, b)
        bound, note = max(KTOL, 4 * spread), f" (torch fp32 maxrel {spread:.2e}, bound {max(KTOL, 4 * spread):.2e})"
    print(f"{what}: nrel {e2:.2e} maxrel {em:.2e}{note}")
    if report is not None:
        report(what, nrel=e2, maxrel=em, **({"fp32_spread": maxrel(a32, b)} if a32 is not None else {}))
    assert e2 < KTOL and em < bound, f"{what}: nrel {e2:.2e} maxrel {em:.2e}{note}"
    return True


def f32(*shape, g, scale=1.0, shift=0.0):
    """fp32-representable random values as fp64"""
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift).float().double()


def nan_buf(n, h, w, c, pad):
    from floodgan.plans import Buf
    B = Buf.empty(n, h, w, c, pad, DEV)
    B.t.fill_(NAN)
    return B


def buf_nan_border(x_nchw, pad, c_alloc=None):
    """buf_from with NaN, not zeros, in the border and in the channels above x's: nothing may read them"""
    from floodgan.plans import Buf
    n, c, h, w = x_nchw.shape
    c_alloc = c_alloc or c
    nhwc = torch.full((n, h + 2 * pad, w + 2 * pad, c_alloc), NAN, dtype=torch.float32)
    nhwc[:, pad:pad + h, pad:pad + w, :c] = x_nchw.float().permute(0, 2, 3, 1)
    return Buf(nhwc.reshape(-1).to(DEV), n, h, w, c_alloc, pad)


def border_still_nan(B):
    """the border of a NaN-prefilled Buf was left alone"""
    t, p = B.nhwc().cpu().clone(), B.pad
    t[:, p:p + B.h, p:p + B.w] = NAN
    return bool(torch.isnan(t).all())


def _ref_fwd(x, groups, gamma, beta, rm, rv, mask):
    """fp64 CPU: sequential BN calls per group (F.batch_norm updates rm / rv in place)"""
    outs = []
    for xg in x.chunk(groups, 0):
        outs.append(F.batch_norm(xg, rm, rv, gamma, beta, training=True, momentum=0.1, eps=1e-5))
    u = torch.cat(outs, 0)
    return u * (mask / 0.5) if mask is not None else u


# (n, c, h, w, groups, dropout).  chunks = min(1024 / groups, HW / 16) (at least 1), per = ceil(HW / chunks)
# pixels per chunk; L = C / 4 lanes per pixel, PG = 256 / L pixels per block step.
CASES = [(2, 64, 8, 8, 1, False), (4, 128, 16, 12, 2, True), (2, 512, 1, 1, 1, False), (2, 512, 2, 2, 1, True),
         (6, 256, 4, 4, 3, False), (1, 64, 64, 64, 1, True), (8, 64, 64, 64, 2, True),
         # HW = 289: 18 chunks of 17; 17 * 17 = 289, so chunk 17 starts at the end and is empty
         (2, 64, 17, 17, 1, False),
         # one image per group; HW = 63: min(341, 3) = 3 chunks of 21; L = 8, PG = 32
         (3, 32, 7, 9, 3, True),
         # C = 4: L = 1, PG = 256; HW = 1023: min(512, 63) = 63 chunks of 17; 60 * 17 = 1020 < 1023 <= 61 * 17, so
         # chunk 60 holds 3 pixels and chunks 61 and 62 start past the end
         (4, 4, 33, 31, 2, False),
         # HW = 16640: HW / 16 = 1040 > MAX_PARTIALS, so 1024 chunks of 17; 978 * 17 = 16626 < 16640 <= 979 * 17:
         # chunk 978 holds 14 pixels, the chunks from 979 on are empty.  4 * 16640 * 16 = 1,064,960 float4s
         # exceed the apply kernels' 4096 x 256 = 1,048,576 grid: a second grid-stride iteration
         (4, 64, 128, 130, 1, True),
         # HW = 25: 1 chunk of 25; eight groups = eight running-statistics updates in order, M = 25
         (8, 16, 5, 5, 8, False),
         # C = 1024 (the segmentation U-Net's bottleneck): L = 256, PG = 1; HW = 15 and 16: 1 chunk
         (2, 1024, 3, 5, 1, True), (4, 1024, 4, 4, 2, False),
         # C = 8: L = 2, PG = 128; HW = 99: 6 chunks of 17, chunk 5 holds 14 pixels
         (2, 8, 9, 11, 1, True)]


# Cases fp32 cannot hold to KTOL in the max norm; their max-norm bound is 4 x torch's own fp32-vs-fp64 distance.
# (2, 512, 1, 1): M = 2 values per channel, and the channel whose two values lie 3.5e-4 apart loses three to four
# digits in x - mean (the mean is an fp32 number); torch CPU float32 is 1.7e-5 from fp64 there, the kernel 2.4e-5.
FP32_LIMITED = {(2, 512, 1, 1, 1)}


def _torch_ref(x, gamma, beta, rm0, rv0, mask, gA, gB, groups, dtype):
    """the forward / backward under test in torch CPU at `dtype`, with autograd"""
    x, gamma, beta, rm, rv, gA, gB = (t.to(dtype).clone() for t in (x, gamma, beta, rm0, rv0, gA, gB))
    xr, gr, br = (t.requires_grad_(True) for t in (x, gamma, beta))
    u = _ref_fwd(xr, groups, gr, br, rm, rv, None if mask is None else mask.to(dtype))
    yA, yB = F.leaky_relu(u, 0.2), F.relu(u)
    dx, dgam, dbet = torch.autograd.grad((yA * gA).sum() + (yB * gB).sum(), (xr, gr, br))
    return dict(yA=yA.detach(), yB=yB.detach(), dx=dx, dgam=dgam, dbet=dbet, rm=rm, rv=rv)


def _forward_backward(n, c, h, w, groups, drop, src_pad=0, g_pad=0, report=None):
    from floodgan import _lib as L
    from floodgan import ops
    from floodgan.plans import Slice

    tag = f"bn {n}x{c}x{h}x{w} g{groups} pad{src_pad}{g_pad}"
    g = torch.Generator().manual_seed(n * 1000 + c + h)
    x = f32(n, c, h, w, g=g, scale=1.7, shift=0.6)
    gamma = f32(c, g=g, scale=0.1, shift=1.0)
    beta = f32(c, g=g, scale=0.1)
    rm0, rv0 = f32(c, g=g, scale=0.3), (1 + torch.rand(c, generator=g, dtype=torch.float64)).float().double()
    mask = torch.empty(n, c, h, w, dtype=torch.float32).bernoulli_(0.5, generator=g) if drop else None
    gA, gB = f32(n, c, h, w, g=g), f32(n, c, h, w, g=g)

    R = _torch_ref(x, gamma, beta, rm0, rv0, mask, gA, gB, groups, torch.float64)
    if (n, c, h, w, groups) in FP32_LIMITED:
        R32 = _torch_ref(x, gamma, beta, rm0, rv0, mask, gA, gB, groups, torch.float32)
    else:
        R32 = dict.fromkeys(R)

    # HIP
    src = buf_nan_border(x, src_pad)
    dA = nan_buf(n, h, w, c, 1)
    wide = nan_buf(n, h, w, 2 * c, 0)
    d_gamma, d_beta = gamma.float().to(DEV), beta.float().to(DEV)
    d_rm, d_rv = rm0.float().to(DEV), rv0.float().to(DEV)
    d_nbt = torch.tensor([7], dtype=torch.int64, device=DEV)
    d_mask = mask.to(DEV) if mask is not None else None
    mean, invstd = ops.bn_stats(src, groups, (d_rm, d_rv, d_nbt))
    ops.bn_apply(src, groups, mean, invstd, d_gamma, d_beta, d_mask, L.FG_ACT_LRELU, dA, L.FG_ACT_RELU,
                 Slice(wide, c, c))
    torch.cuda.synchronize()
    close(tag + " lrelu", nchw(dA), R["yA"], report, R32["yA"])
    close(tag + " relu slice", wide.interior()[..., c:].permute(0, 3, 1, 2).cpu(), R["yB"], report, R32["yB"])
    assert bool(torch.isnan(wide.interior()[..., :c]).all())             # the other half untouched
    assert border_still_nan(dA)                                           # border untouched
    close(tag + " running_mean", d_rm.cpu(), R["rm"], report, R32["rm"])
    close(tag + " running_var", d_rv.cpu(), R["rv"], report, R32["rv"])
    assert int(d_nbt) == 7 + groups                                       # num_batches_tracked: one per group

    # backward: gA through LeakyReLU, gB (a channel slice; the other half is NaN) through ReLU
    gAb = buf_nan_border(gA, g_pad)
    gwide = buf_from(torch.cat((torch.full_like(gB, NAN), gB), 1), 0, "constant")
    dst = nan_buf(n, h, w, c, 1)
    gg, gb = torch.full((c,), NAN, device=DEV), torch.full((c,), NAN, device=DEV)
    ops.bn_bwd(gAb, L.FG_ACT_LRELU, Slice(gwide, c, c), L.FG_ACT_RELU, src, groups, mean, invstd, d_gamma, d_beta,
               d_mask, dst, gg, gb, accumulate=False)
    torch.cuda.synchronize()
    close(tag + " dx", nchw(dst), R["dx"], report, R32["dx"])
    assert border_still_nan(dst)
    close(tag + " dgamma", gg.cpu(), R["dgam"], report, R32["dgam"])
    close(tag + " dbeta", gb.cpu(), R["dbet"], report, R32["dbet"])
    # accumulate adds onto the existing gradients
    ops.bn_bwd(gAb, L.FG_ACT_LRELU, Slice(gwide, c, c), L.FG_ACT_RELU, src, groups, mean, invstd, d_gamma, d_beta,
               d_mask, dst, gg, gb, accumulate=True)
    torch.cuda.synchronize()
    close(tag + " dgamma x2", gg.cpu(), 2 * R["dgam"], report, None if R32["dgam"] is None else 2 * R32["dgam"])
    close(tag + " dbeta x2", gb.cpu(), 2 * R["dbet"], report, None if R32["dbet"] is None else 2 * R32["dbet"])


@pytest.mark.parametrize("n,c,h,w,groups,drop", CASES)
def test_bn_forward_backward(n, c, h, w, groups, drop, report):
    _forward_backward(n, c, h, w, groups, drop, report=report)


def test_bn_padded_source_and_gradient(report):
    """source and incoming gradient with a 1-wide border (NaN in it): every read goes through the padded index"""
    _forward_backward(2, 64, 17, 17, 1, True, src_pad=1, g_pad=1, report=report)
    _forward_backward(3, 32, 7, 9, 3, False, src_pad=1, g_pad=1, report=report)


def test_bn_num_batches_tracked():
    """an int64 third running entry rises by `groups` per launch, exactly (nn.BatchNorm2d counts calls)"""
    from floodgan import ops

    g = torch.Generator().manual_seed(21)
    src = buf_from(f32(6, 8, 5, 5, g=g), 0, "constant")
    rm, rv = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    nbt = torch.tensor([2 ** 40 + 5], dtype=torch.int64, device=DEV)
    for groups in (1, 3, 6):
        ops.bn_stats(src, groups, (rm, rv, nbt))
    torch.cuda.synchronize()
    assert int(nbt) == 2 ** 40 + 5 + 1 + 3 + 6


def test_bn_large_mean_stats(report):
    """a channel whose mean dwarfs its spread: the shifted sums keep mean and invstd at the kernel bound
    (unshifted fp32 sums of x^2 ~ 9e4 could not resolve a variance of 1e-4); a ragged chunk tail as well"""
    from floodgan import ops

    g = torch.Generator().manual_seed(22)
    x = f32(2, 8, 9, 11, g=g, scale=0.01, shift=300.0)
    mean, invstd = ops.bn_stats(buf_nan_border(x, 1), 1)
    torch.cuda.synchronize()
    var = x.var(dim=(0, 2, 3), unbiased=False)
    close("bn large-mean mean", mean.cpu(), x.mean(dim=(0, 2, 3)), report)
    close("bn large-mean invstd", invstd.cpu(), 1 / torch.sqrt(var + 1e-5), report)


@pytest.mark.parametrize("c", [1, 255, 256, 257])
def test_bn_eval_stats(c):
    """module.eval(): mean is running_mean bit for bit, invstd = 1 / sqrt(running_var + float32(1e-5)) within one
    fp32 ulp, at running_var 0 and 1e-12 too; nothing is written past channel c - 1"""
    from floodgan import _lib as L

    g = torch.Generator().manual_seed(c)
    eps = torch.tensor(1e-5, dtype=torch.float32).double()
    for first, last in ((0.0, 1e-12), (1e-12, 0.0)):
        rm = torch.randn(c, generator=g)
        rv = torch.rand(c, generator=g) * 3
        rv[-1], rv[0] = last, first
        d_rm, d_rv = rm.to(DEV), rv.to(DEV)
        mean, invstd = torch.full((c + 64,), NAN, device=DEV), torch.full((c + 64,), NAN, device=DEV)
        L.check(L.load().fg_bn_eval_stats(c, L.ptr(d_rm), L.ptr(d_rv), C.c_float(1e-5), L.ptr(mean), L.ptr(invstd),
                                          L.stream_handle()), "bn_eval_stats")
        torch.cuda.synchronize()
        assert torch.equal(mean[:c].cpu(), rm)
        ref = 1 / torch.sqrt(rv.double() + eps)
        ref32 = ref.float()
        ulp = (torch.nextafter(ref32, torch.full_like(ref32, float("inf"))) - ref32).double()
        assert bool(((invstd[:c].cpu().double() - ref).abs() <= ulp).all())
        assert bool(torch.isnan(mean[c:]).all()) and bool(torch.isnan(invstd[c:]).all())


def test_bn_eval_stats_wrapper():
    from floodgan import ops

    rm, rv = torch.randn(64).to(DEV), torch.rand(64).to(DEV)
    mean, invstd = ops.bn_eval_stats(rm, rv)
    torch.cuda.synchronize()
    assert torch.equal(mean, rm)
    close("bn eval invstd", invstd.cpu(), 1 / torch.sqrt(rv.cpu().double() + 1e-5))


def test_bn_identity_mode_and_large_mean():
    """mean=None: activation only (the U-Net's un-normalised outermost / innermost downs); a channel
    whose mean dwarfs its spread (shifted sums keep the variance accurate)"""
    from floodgan import _lib as L
    from floodgan import ops
    from floodgan.plans import Buf

    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 32, 32, generator=g, dtype=torch.float64)
    src = buf_from(x, 0, "constant")
    d0, d1 = Buf.zeros(2, 32, 32, 64, 1, DEV), Buf.zeros(2, 32, 32, 64, 1, DEV)
    ops.bn_apply(src, 1, None, None, None, None, None, L.FG_ACT_LRELU, d0, L.FG_ACT_RELU, d1)
    torch.cuda.synchronize()
    assert nrel(nchw(d0), F.leaky_relu(x, 0.2)) < KTOL and nrel(nchw(d1), F.relu(x)) < KTOL
    gA = torch.randn(2, 64, 32, 32, generator=g, dtype=torch.float64)
    dst = Buf.zeros(2, 32, 32, 64, 1, DEV)
    ops.bn_bwd(buf_from(gA, 0, "constant"), L.FG_ACT_RELU, None, 0, src, 1, None, None, None, None, None, dst)
    torch.cuda.synchronize()
    assert nrel(nchw(dst), gA * (x > 0)) < KTOL

    xb = x * 0.01 + 300.0
    srcb = buf_from(xb, 0, "constant")
    mean, invstd = ops.bn_stats(srcb, 1)
    torch.cuda.synchronize()
    var = xb.var(dim=(0, 2, 3), unbiased=False)
    assert nrel(mean.cpu(), xb.mean(dim=(0, 2, 3))) < 1e-7
    assert nrel(invstd.cpu(), 1 / torch.sqrt(var + 1e-5)) < 1e-4


def test_bn_identity_mode_exact_zeros(report):
    """mean=None with exact zeros (and -0.0) in the source: ReLU'(0) = 0 and LeakyReLU'(0) = 0.2, torch's
    convention, so the fp64 autograd reference decides every element the same way"""
    from floodgan import _lib as L
    from floodgan import ops

    g = torch.Generator().manual_seed(23)
    n, c, h, w = 2, 8, 9, 11
    x = f32(n, c, h, w, g=g)
    x.view(-1)[::3] = 0.0
    x.view(-1)[1::30] = -0.0
    gA, gB = f32(n, c, h, w, g=g), f32(n, c, h, w, g=g)
    xr = x.clone().requires_grad_(True)
    yA, yB = F.relu(xr), F.leaky_relu(xr, 0.2)
    (dx,) = torch.autograd.grad((yA * gA).sum() + (yB * gB).sum(), xr)
    assert bool((dx[x == 0] == 0.2 * gB[x == 0]).all())                 # the convention itself
    src = buf_nan_border(x, 1)
    d0, d1 = nan_buf(n, h, w, c, 1), nan_buf(n, h, w, c, 0)
    ops.bn_apply(src, 1, None, None, None, None, None, L.FG_ACT_RELU, d0, L.FG_ACT_LRELU, d1)
    dst = nan_buf(n, h, w, c, 1)
    ops.bn_bwd(buf_nan_border(gA, 0), L.FG_ACT_RELU, buf_nan_border(gB, 1), L.FG_ACT_LRELU, src, 1, None, None, None,
               None, None, dst)
    torch.cuda.synchronize()
    close("bn identity relu", nchw(d0), yA, report)
    close("bn identity lrelu", nchw(d1), yB, report)
    close("bn identity dx", nchw(dst), dx, report)
    assert border_still_nan(d0) and border_still_nan(dst)
    assert bool((nchw(d0)[x == 0] == 0).all()) and bool((nchw(d1)[x == 0] == 0).all())


REJECTED = [(2, 48, 4, 4, 1),       # L = 12: 256 % 12 != 0
            (2, 2048, 2, 2, 1),     # L = 512 lanes do not fit a 256-thread block
            (3, 64, 4, 4, 2)]       # n % groups != 0


@pytest.mark.parametrize("n,c,h,w,groups", REJECTED)
def test_bn_rejects_unsupported(n, c, h, w, groups):
    """fg_bn_stats and fg_bn_bwd refuse a channel count their thread layout cannot walk and a batch the groups do
    not divide -- and write nothing"""
    from floodgan import _lib as L
    from floodgan import ops

    g = torch.Generator().manual_seed(24)
    src = buf_from(f32(n, c, h, w, g=g), 0, "constant")
    outs = [torch.full((groups * c,), NAN, device=DEV) for _ in range(4)]
    mean, invstd, rm, rv = outs
    nbt = torch.tensor([3], dtype=torch.int64, device=DEV)
    work = ops._bn_work(n, c, DEV)
    with pytest.raises(RuntimeError, match="fg_bn_stats"):
        L.check(L.load().fg_bn_stats(ops.view(src), groups, C.c_float(1e-5), C.c_float(0.1), L.ptr(mean),
                                     L.ptr(invstd), L.ptr(rm), L.ptr(rv), L.ptr(nbt), L.ptr(work), L.stream_handle()),
                "bn_stats")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs) and int(nbt) == 3
    with pytest.raises(RuntimeError, match="fg_bn_stats"):
        ops.bn_stats(src, groups, (rm, rv, nbt))

    m, s = torch.zeros(groups * c, device=DEV), torch.ones(groups * c, device=DEV)
    gam, bet = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    dst = nan_buf(n, h, w, c, 1)
    gg, gb = torch.full((c,), NAN, device=DEV), torch.full((c,), NAN, device=DEV)
    with pytest.raises(RuntimeError, match="fg_bn_bwd"):
        ops.bn_bwd(src, L.FG_ACT_RELU, None, 0, src, groups, m, s, gam, bet, None, dst, gg, gb)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dst.t, gg, gb))


# the second shape is the one at which bn_apply_kernel / bn_bwd_apply_kernel take a second grid-stride iteration
@pytest.mark.parametrize("n,c,h,w", [(2, 64, 9, 11), (4, 64, 128, 130)])
def test_bn_absmax_slots(f16x3, n, c, h, w):
    """fg_bn_apply raises one absmax slot per destination and fg_bn_bwd one for dst: each equals the maximum of what
    was written there.  act0 = ReLU and act1 = none over data whose negative side is ten times its positive side puts
    max |dst1| far above max |dst0|: a dst1 value that leaked into slot 0 (the two flushes share one LDS array) shows."""
    from floodgan import _lib as L
    from floodgan import ops
    from floodgan.plans import Slice

    assert L.fwd_f16x3()
    g = torch.Generator().manual_seed(25)
    x = f32(n, c, h, w, g=g)
    x = torch.where(x < 0, 10 * x, x).float().double()
    src = buf_from(x, 0, "constant")
    gamma, beta = f32(c, g=g, scale=0.1, shift=1.0).float().to(DEV), f32(c, g=g, scale=0.1).float().to(DEV)
    mean, invstd = ops.bn_stats(src, 1)
    d0, wide = nan_buf(n, h, w, c, 0), nan_buf(n, h, w, 2 * c, 0)
    slot = ops.amax_slot(wide)
    ops.bn_apply(src, 1, mean, invstd, gamma, beta, None, L.FG_ACT_RELU, d0, L.FG_ACT_NONE, Slice(wide, c, c),
                 slots=(None, slot))
    torch.cuda.synchronize()
    m0, m1 = float(d0.t.abs().max()), float(wide.interior()[..., c:].abs().max())
    assert m1 > 2 * m0 > 0                                                # the data does separate the two
    assert float(ops.slot_of(d0).max()) == m0
    assert ops.slot_of(wide) is slot and float(slot.max()) == m1
    assert bool(torch.isnan(wide.interior()[..., :c]).all())

    dst = nan_buf(n, h, w, c, 0)
    ops.bn_bwd(buf_from(f32(n, c, h, w, g=g), 0, "constant"), L.FG_ACT_RELU, None, 0, src, 1, mean, invstd, gamma,
               beta, None, dst)
    torch.cuda.synchronize()
    assert float(ops.slot_of(dst).max()) == float(dst.t.abs().max()) > 0


@pytest.mark.parametrize("h,w", [(16, 16), (7, 9), (2, 2)])
def test_maxpool2(h, w):
    from floodgan import ops
    from floodgan.plans import Buf

    x = torch.randn(3, 128, h, w, dtype=torch.float64, generator=torch.Generator().manual_seed(h * w))
    dst = Buf.zeros(3, h // 2, w // 2, 128, 1, DEV)
    ops.maxpool2(buf_from(x, 1, "constant"), dst)
    torch.cuda.synchronize()
    assert torch.equal(nchw(dst).double(), F.max_pool2d(x.float(), 2).double())


def test_hashed_dropout_equals_its_mask():
    """Device dropout (keep decisions hashed from (seed, NCHW index), recomputed in the backward) gives
    exactly the result of the same decisions passed as a mask; the decisions are Bernoulli(0.5):
    the kept fraction and its independence across seeds / neighbouring elements."""
    from floodgan import _lib as L
    from floodgan import ops
    from floodgan.plans import Buf

    g = torch.Generator().manual_seed(11)
    n, c, h, w = 2, 512, 16, 16
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    gA = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    gamma, beta = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    src = buf_from(x, 0, "constant")
    seed = 0x1234_5678_9ABC
    mask = ops.dropout_mask(seed, (n, c, h, w), DEV)
    outs = []
    for drop in (seed, mask):
        mean, invstd = ops.bn_stats(src, 1)
        d = Buf.zeros(n, h, w, c, 1, DEV)
        ops.bn_apply(src, 1, mean, invstd, gamma, beta, drop, L.FG_ACT_RELU, d)
        gd = Buf.zeros(n, h, w, c, 1, DEV)
        ops.bn_bwd(buf_from(gA, 0, "constant"), L.FG_ACT_RELU, None, 0, src, 1, mean, invstd, gamma, beta, drop, gd)
        torch.cuda.synchronize()
        outs.append((nchw(d), nchw(gd)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    m = mask.cpu().double()
    assert set(m.unique().tolist()) == {0.0, 1.0}
    assert abs(float(m.mean()) - 0.5) < 0.005                                # 262144 draws: sd 0.001
    m2 = ops.dropout_mask(seed + 1, (n, c, h, w), DEV).cpu().double()
    assert abs(float(((m - 0.5) * (m2 - 0.5)).mean())) < 0.005              # seeds independent
    assert abs(float(((m[..., 1:] - 0.5) * (m[..., :-1] - 0.5)).mean())) < 0.005   # neighbours independent
