"""The flood-mask loss on the device (floodgan.segmentation.FloodMaskLoss): its three kernels at their edges against
fp64 torch on the CPU (fg_bn_bwd_fixed, fg_unit_image_bwd, fg_flood_mask_bce), the U-Net's input gradient and its
eval-mode backward against the teacher-forced fp64 oracle (tests/seg_train_oracle.py), the module under stock
autograd, and the opt-in term of the fused paired step.

Bounds.  fg_bn_bwd_fixed's input gradient: 5e-7 of the largest element (at most four fp32 roundings, 2^-24 each);
its parameter gradients: KTOL in both norms, what tests/test_gpu_bnorm.py holds for fg_bn_bwd's.  fg_unit_image_bwd:
bit-equal to ATen where no rounding can differ, else one fp32 rounding (2^-24 relative) of fp64.  fg_flood_mask_bce:
1e-6 for loss and gradient, what tests/test_gpu_seg_train.py holds for fg_bce_logits.  U-Net gradients: 1e-4, what
test_unet_backward_teacher_forced holds for every parameter gradient (inc's are the end of the chain the input
gradient continues by one conv)."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

import seg_train_oracle as SO
from test_gpu_bnorm import border_still_nan, buf_nan_border, close, f32, maxrel, nan_buf
from test_gpu_northstar import KINK
from test_gpu_parity import DEV, buf_from, nchw, nrel
from test_gpu_seg_train import _batch, _init_module

pytestmark = pytest.mark.gpu

NAN = float("nan")
ULP = 2.0 ** -24            # half a unit in the last place, relative: one correct fp32 rounding


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from floodgan import _lib as L
    L.check(L.load().fg_device_ok(), "device_ok")
    torch.set_num_threads(min(16, max(1, len(os.sched_getaffinity(0)))))


def device_flood(t):
    """the device's own flood decision (fg::flood, through the renderer's "logit" kind) of channel 0 of an NHWC Buf
    or an [N, 1, H, W] device tensor: bool [N, H, W] on the host"""
    from floodgan import ops
    from floodgan.plans import Buf
    n, h, w = (t.n, t.h, t.w) if isinstance(t, Buf) else (t.shape[0], t.shape[2], t.shape[3])
    lut = torch.zeros(256, 4, dtype=torch.uint8, device=DEV)
    lut[255] = 255
    canvas = torch.zeros(n * h, w, 4, dtype=torch.uint8, device=DEV)
    ops.render_scalar(t, lut, canvas, kind="logit", step_rows=h)
    return canvas[..., 0].reshape(n, h, w).cpu() > 0


# ------------------------------------------------------------------------------------------ fg_bn_bwd_fixed

# (N, H, W, C): an odd plane smaller than the chunking; the bottleneck of a 32^2 input (C / 4 = the block);
# two images of 64 pixels (4 chunks of 16)
FIXED_SHAPES = [(2, 3, 5, 64), (1, 2, 2, 1024), (2, 8, 8, 128)]


def _fixed_case(n, h, w, c, second):
    """fp32-representable inputs whose every ReLU gate is decided far from rounding, and the fp64 gradients"""
    g = torch.Generator().manual_seed(n * 1000 + c + h + int(second))
    x = f32(n, c, h, w, g=g, scale=1.7, shift=0.6)
    gamma, beta = f32(c, g=g, scale=0.1, shift=1.0), f32(c, g=g, scale=0.1)
    mean = f32(c, g=g, scale=0.3)
    invstd = (1 / torch.sqrt(0.5 + torch.rand(c, generator=g, dtype=torch.float64))).float().double()
    v = lambda t: t.view(1, c, 1, 1)                                             # noqa: E731
    u = (x - v(mean)) * v(invstd) * v(gamma) + v(beta)
    x = torch.where(u.abs() < 1e-3, x + 0.05, x).float().double()                # move the few gates near the kink
    gA = f32(n, c, h, w, g=g)
    gB = f32(n, c, h, w, g=g) if second else None
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    xhat = (xr - v(mean)) * v(invstd)
    ur = xhat * v(gr) + v(br)
    assert float(ur.detach().abs().min()) > 1e-4
    y = F.relu(ur)
    dx, dgam, dbet = torch.autograd.grad((y * gA).sum() + ((y * gB).sum() if second else 0), (xr, gr, br))
    return dict(x=x, gamma=gamma, beta=beta, mean=mean, invstd=invstd, gA=gA, gB=gB, dx=dx, dgam=dgam, dbet=dbet)


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("shape", FIXED_SHAPES)
def test_bn_bwd_fixed_vs_fp64(shape, second, report):
    from floodgan import _lib as L
    from floodgan import ops
    n, h, w, c = shape
    R = _fixed_case(n, h, w, c, second)
    dev = {k: R[k].float().to(DEV) for k in ("gamma", "beta", "mean", "invstd")}
    src, gA = buf_nan_border(R["x"], 1), buf_nan_border(R["gA"], 0)
    gB = buf_nan_border(R["gB"], 1) if second else None
    actB = L.FG_ACT_RELU if second else 0
    worst = 0.0
    for pad in (0, 1):
        for params in (False, True):
            for acc in (False, True):
                dst = nan_buf(n, h, w, c, pad)
                gg = gb = None
                if params:
                    gg = torch.full((c,), 3.0 if acc else NAN, device=DEV)
                    gb = torch.full((c,), -2.0 if acc else NAN, device=DEV)
                ops.bn_bwd_fixed(gA, L.FG_ACT_RELU, gB, actB, src, dev["mean"], dev["invstd"], dev["gamma"],
                                 dev["beta"], dst, gg, gb, accumulate=acc)
                assert L.last_launch() == "bn_bwd_fixed_apply"
                e = maxrel(nchw(dst), R["dx"])
                worst = max(worst, e)
                tag = f"bn_bwd_fixed {shape} second {second} pad {pad} params {params} acc {acc}"
                print(f"{tag}: dx maxrel {e:.2e}")
                assert e <= 5e-7, (tag, e)
                assert border_still_nan(dst), tag
                if params:
                    close(tag + " dgamma", gg.cpu(), R["dgam"] + (3.0 if acc else 0.0))
                    close(tag + " dbeta", gb.cpu(), R["dbet"] - (2.0 if acc else 0.0))
    report("bn_bwd_fixed", shape=list(shape), second=second, dx_maxrel=worst)


def test_bn_bwd_fixed_rejects_bad_arguments():
    from floodgan import _lib as L
    from floodgan import ops
    n, h, w, c = 2, 4, 4, 64
    ok = lambda cc=c, hh=h: buf_from(torch.ones(n, cc, hh, w), 0, "constant")    # noqa: E731
    vec = torch.ones(c, device=DEV)
    dst = nan_buf(n, h, w, c, 0)
    gg, gb = torch.full((c,), NAN, device=DEV), torch.full((c,), NAN, device=DEV)
    # a null source (below the wrapper, which would refuse it first)
    rc = L.load().fg_bn_bwd_fixed(ops.view(ok()), 1, ops.view(None), 0, ops.view(None), L.ptr(vec), L.ptr(vec),
                                  L.ptr(vec), L.ptr(vec), ops.view(dst), L.ptr(gg), L.ptr(gb), 0, None, None,
                                  L.stream_handle())
    assert rc != 0 and b"fg_bn_bwd_fixed" in L.load().fg_last_error()
    with pytest.raises(RuntimeError, match="fg_bn_bwd_fixed"):                  # the gradient on another grid
        ops.bn_bwd_fixed(ok(hh=h + 1), 1, None, 0, ok(), vec, vec, vec, vec, dst, gg, gb)
    with pytest.raises(RuntimeError, match="fg_bn_bwd_fixed"):                  # the second gradient on another grid
        ops.bn_bwd_fixed(ok(), 1, ok(hh=h + 1), 1, ok(), vec, vec, vec, vec, dst, gg, gb)
    with pytest.raises(RuntimeError, match="fg_bn_bwd_fixed"):                  # no statistics
        ops.bn_bwd_fixed(ok(), 1, None, 0, ok(), None, vec, vec, vec, dst)
    v48, d48 = torch.ones(48, device=DEV), nan_buf(n, h, w, 48, 0)
    with pytest.raises(RuntimeError, match="fg_bn_bwd_fixed"):                  # C / 4 = 12 does not divide the block
        ops.bn_bwd_fixed(ok(48), 1, None, 0, ok(48), v48, v48, v48, v48, d48)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dst.t, d48.t, gg, gb))      # nothing was written


# ------------------------------------------------------------------------------------------ fg_unit_image_bwd

def _special_image(W, seed):
    """[2, 3, 4, W] in about [-1.5, 1.5] holding -1, +1, their two fp32 neighbours on each side, 0, NaN, +-inf"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((2, 3, 4, W), generator=g) * 3 - 1.5
    sp = [0.0, NAN, float("inf"), -float("inf")]
    for v in (-1.0, 1.0):
        t = torch.tensor(v)
        sp.append(v)
        for towards in (10.0, -10.0):
            a = torch.nextafter(t, torch.tensor(towards))
            sp += [float(a), float(torch.nextafter(a, torch.tensor(towards)))]
    assert len(sp) == 14
    flat = x.view(-1)
    for i, v in enumerate(sp):                           # every special value in both images
        flat[3 * i + 1] = v
        flat[x[0].numel() + 2 * i] = v
    return x


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("W", [5, 8])
def test_unit_image_bwd(W, channels_last):
    from floodgan import ops
    x = _special_image(W, 70 + W)
    N, C, H, _ = x.shape
    g = torch.randn((N, C, H, W), generator=torch.Generator().manual_seed(71))
    xr = x.clone().requires_grad_(True)
    torch.clamp((xr + 1) * 0.5, 0, 1).backward(g)
    ref32 = xr.grad
    gate = (ref32 != 0).double()
    assert 0 < int(gate.sum()) < gate.numel()
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    xd = x.to(DEV).contiguous(memory_format=fmt)
    G = buf_nan_border(g, 1, 4)                                           # border and channel 3: never read
    for scale in (1.0, 0.3):
        for acc in (False, True):
            d0 = torch.randn((N, C, H, W), generator=torch.Generator().manual_seed(72))
            dst = (d0 if acc else torch.full_like(d0, NAN)).to(DEV).contiguous(memory_format=fmt)
            ops.unit_image_bwd(G, xd, dst, scale=scale, accumulate=acc)
            got = dst.cpu()
            assert not torch.isnan(got).any()
            if scale == 1.0 and not acc:
                assert torch.equal(got, ref32)                            # the factor 0.5 is exact
            s32 = float(torch.tensor(scale, dtype=torch.float32))
            ref = (d0.double() if acc else 0) + s32 * 0.5 * g.double() * gate
            err = (got.double() - ref).abs()
            worst = float((err / ref.abs().clamp_min(1e-30)).max())
            assert bool((err <= ULP * ref.abs() + 1e-45).all()), (scale, acc, worst)


def test_unit_image_bwd_is_validated():
    from floodgan import ops
    x = torch.zeros(2, 3, 4, 8, device=DEV)
    with pytest.raises(RuntimeError, match="unit_image_bwd"):
        ops.unit_image_bwd(buf_from(torch.zeros(2, 3, 4, 8), 0, "constant", 4), x, torch.zeros(2, 3, 4, 4, device=DEV))
    with pytest.raises(RuntimeError, match="fg_unit_image_bwd"):              # the gradient on another grid
        ops.unit_image_bwd(buf_from(torch.zeros(2, 3, 8, 8), 0, "constant", 4), x, torch.zeros_like(x))


# ------------------------------------------------------------------------------------------ fg_flood_mask_bce

def _special_logits():
    sp = [0.0, 100.0, -100.0]
    for v in (2.0 ** -21, -2.0 ** -21):
        t = torch.tensor(v)
        sp += [v, float(torch.nextafter(t, torch.tensor(1.0))), float(torch.nextafter(t, torch.tensor(-1.0)))]
    return sp


def _mask_bce_cases(H, W):
    """(z, r) pairs [2, 1, H, W]: image 0 walks every (special, special) pair, image 1 is a plane of all-equal
    logits against random ones; as many cases as the grid needs to hold all pairs"""
    sp = _special_logits()
    pairs = [(a, b) for a in sp for b in sp]
    g = torch.Generator().manual_seed(80 + H)
    cases = []
    for i0 in range(0, len(pairs), H * W):
        z, r = torch.randn((2, 1, H, W), generator=g) * 3, torch.randn((2, 1, H, W), generator=g) * 3
        chunk = pairs[i0:i0 + H * W]
        z[0].view(-1)[:len(chunk)] = torch.tensor([a for a, _ in chunk])
        r[0].view(-1)[:len(chunk)] = torch.tensor([b for _, b in chunk])
        z[1] = sp[(i0 // (H * W)) % len(sp)]
        # the plane's targets disagree with it, so its loss is log 2 .. 100 and the mean is never a denormal (a
        # pair such as (100, 100) alone has the loss 3.7e-44, which no fp32 sum holds to a relative bound)
        r[1] = r[1].abs().clamp_min(0.01) * (-1.0 if float(z[1, 0, 0, 0]) > 0 else 1.0)
        cases.append((z, r))
    return cases


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (16, 16)])
def test_flood_mask_bce(H, W, report):
    from floodgan import ops
    from floodgan.evaluate import MaskConfusion
    from floodgan.plans import Buf
    N = 2
    gscale = 0.7 / (N * H * W)
    worst = [0.0, 0.0]
    for z, r in _mask_bce_cases(H, W):
        Z, Rr = buf_from(z, 1, "constant", 4), buf_from(r, 0, "constant", 8)     # different borders and strides
        Z.nhwc()[..., 1:] = 7.0
        Rr.nhwc()[..., 1:] = -7.0                                                 # only channel 0 is read
        grad = Buf(torch.full((N * (H + 2) * (W + 2) * 4,), NAN, device=DEV), N, H, W, 4, 1)
        res = torch.zeros(2, dtype=torch.int64, device=DEV)
        ops.flood_mask_bce(Z, Rr, gscale, grad, res)
        conf = MaskConfusion(DEV)
        conf.update(Z, Rr)
        tp, fp, tn, fn = (int(v) for v in conf.counts.cpu())
        res = res.cpu()
        assert int(res[1]) == tp + tn, (int(res[1]), tp, tn)                      # exactly MaskConfusion's agreement
        t = device_flood(Rr)[:, None].double()                                    # the device's own targets
        assert torch.equal(device_flood(Rr), r[:, 0] > 0)                         # (and they are the sign of r here)
        assert int(t.sum()) == tp + fn
        z64 = z.double()
        loss_ref = float(F.binary_cross_entropy_with_logits(z64, t))
        g_ref = (torch.sigmoid(z64) - t) * gscale
        gr = grad.nhwc().cpu()
        loss = float(res[:1].view(torch.float32)[0])
        e_loss, e_grad = abs(loss - loss_ref) / loss_ref, nrel(gr[:, 1:-1, 1:-1, 0], g_ref[:, 0])
        worst = [max(worst[0], e_loss), max(worst[1], e_grad)]
        assert loss == loss and abs(loss) < 1e30                                  # softplus(100) did not overflow
        assert e_loss < 1e-6 and e_grad < 1e-6, (e_loss, e_grad)
        assert not torch.isnan(gr).any() and float(gr[..., 1:].abs().max()) == 0.0
        border = gr.clone()
        border[:, 1:-1, 1:-1] = 0
        assert float(border.abs().max()) == 0.0
    print(f"flood_mask_bce {H}x{W}: worst loss rel {worst[0]:.2e}, gradient nrel {worst[1]:.2e}")
    report("flood_mask_bce", grid=[H, W], loss_rel=worst[0], grad_nrel=worst[1])


def test_flood_mask_bce_is_validated():
    from floodgan import ops
    from floodgan.plans import Buf
    z, g = Buf.zeros(2, 4, 4, 4, 0, DEV), Buf.zeros(2, 4, 4, 4, 0, DEV)
    res = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="fg_flood_mask_bce"):
        ops.flood_mask_bce(z, Buf.zeros(2, 4, 8, 4, 0, DEV), 1.0, g, res)
    with pytest.raises(RuntimeError, match="int64"):
        ops.flood_mask_bce(z, z, 1.0, g, torch.zeros(4, dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------------------------------ U-Net gradients

def _perturbed_module(seed):
    """seeded initialise_weights; running statistics moved away from (0, 1) so that eval mode is not the identity"""
    net = _init_module(seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, b in net.named_buffers():
            if k.endswith("running_mean"):
                b.add_(torch.randn(b.shape, generator=g) * 0.05)
            elif k.endswith("running_var"):
                b.mul_(0.5 + torch.rand(b.shape, generator=g))
    return net


def _hip_unet_grads(net, x, t, training):
    """executor forward (save=True) + fg_bce_logits + unet_backward(input_grad=True): (grads, decisions, logits, S)"""
    from floodgan import ops
    from floodgan import segmentation as S
    from floodgan.plans import Buf
    P, B = dict(net.named_parameters()), dict(net.named_buffers())
    N, _, H, W = x.shape
    with torch.no_grad():
        logits, saved = S.unet_logits(P, B, S.unit_image_passthrough(x.to(DEV))[1], training, save=True,
                                      update_running=False)
        res = torch.zeros(2, dtype=torch.int64, device=DEV)
        g = Buf.empty(N, H, W, 4, 0, DEV)
        ops.bce_logits(logits, t.to(DEV), 1.0 / t.numel(), g, res[:1].view(torch.float32), res[1:])
        choices = {}
        grads = S.unet_backward(P, saved, g, choices=choices, input_grad=True)
    dec = SO.Decisions(relu=S.unet_decisions(saved), pool={k: v.cpu() for k, v in choices.items()})
    return grads, dec, g, saved


def _oracle_grads(cpu, x, t, training, dec, dtype=torch.float64, device="cpu"):
    P = {k: v.detach().to(device, dtype).requires_grad_(True) for k, v in cpu.named_parameters()}
    B = {k: (v.detach().to(device, dtype) if v.is_floating_point() else v.detach().clone().to(device))
         for k, v in cpu.named_buffers()}
    xr = x.to(device, dtype).requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(SO.unet_forward(P, B, xr, training, dec), t.to(device, dtype))
    keys = list(P)
    gs = torch.autograd.grad(loss, [xr] + [P[k] for k in keys])
    return dict(zip(["input"] + keys, gs))


# (training, N, H, W): eval mode at 16x16 has a 1x1 bottleneck, legal only without batch statistics
UNET_CASES = [(True, 2, 32, 32), (True, 2, 16, 48), (False, 1, 16, 16), (False, 2, 16, 48)]


@pytest.mark.parametrize("training,N,H,W", UNET_CASES)
def test_unet_input_gradient_and_eval_backward_teacher_forced(training, N, H, W, report):
    from floodgan import segmentation as S
    cpu = _perturbed_module(25)
    net = copy.deepcopy(cpu).to(DEV)
    before = {k: v.detach().clone() for k, v in net.named_buffers()}
    x, t = _batch(N, H, W, 33)
    grads, dec, g, saved = _hip_unet_grads(net, x, t, training)
    ref = _oracle_grads(cpu, x, t, training, dec)
    assert set(grads) == set(ref)
    g_in = nchw(grads["input"], 3)
    rows = sorted(((k, nrel(g_in if k == "input" else grads[k], ref[k])) for k in ref), key=lambda r: -r[1])
    e_in = dict(rows)["input"]
    print(f"unet {'train' if training else 'eval'} {N}x{H}x{W}: input gradient nrel {e_in:.2e}; worst {rows[:3]}; "
          f"{dec.differing()} decisions differ, worst kink {dec.worst():.2e}")
    report("seg_unet_input_gradient", training=training, shape=[N, H, W], input_nrel=e_in, worst=rows[0],
           worst_kink=dec.worst())
    assert dec.worst() < KINK, [r for r in dec.log if r[2]]
    assert e_in < 1e-4, e_in
    assert rows[0][1] < 1e-4, rows[:5]                    # every parameter gradient, in eval mode as in train mode
    assert float(ref["input"].abs().max()) > 0
    for k, v in net.named_buffers():                      # (update_running=False: the statistics were left alone)
        assert torch.equal(v, before[k]), k
    # the frozen form: the save="input" state, no parameter gradients, the same input gradient bit for bit
    P, B = dict(net.named_parameters()), dict(net.named_buffers())
    with torch.no_grad():
        _, lean = S.unet_logits(P, B, S.unit_image_passthrough(x.to(DEV))[1], training, save="input",
                                update_running=False)
        for D in lean["enc"] + lean["dec"]:
            assert not {"x", "a", "xin"} & set(D), sorted(D)
            assert {"t", "u", "m1", "i1", "m2", "i2"} <= set(D)
        assert all("out" in D for D in lean["enc"][:4])   # the max-pool sources
        frozen = S.unet_backward(P, lean, g, input_grad=True, param_grads=False)
        assert list(frozen) == ["input"]
        assert torch.equal(nchw(frozen["input"], 3), g_in)
        with pytest.raises(RuntimeError, match="save=\"input\""):
            S.unet_backward(P, lean, g)
    if not training:
        assert torch.equal(saved["enc"][0]["m1"].cpu(), cpu.inc.double_conv[1].running_mean)


# ------------------------------------------------------------------------------------------ FloodMaskLoss

def _images(seed, N=2, R=32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((N, 3, R, R), generator=g) * 2.4 - 1.2).to(DEV), \
        (torch.rand((N, 3, R, R), generator=g) * 2.4 - 1.2).to(DEV)          # some values clamp


def _by_hand(net, fake, real, batch_stats):
    """the loss's pieces called one by one: (loss, agreeing pixels, d loss / d fake)"""
    from floodgan import ops
    from floodgan import segmentation as S
    from floodgan.plans import Buf
    P, B = dict(net.named_parameters()), dict(net.named_buffers())
    N, _, H, W = fake.shape
    with torch.no_grad():
        F0, R0 = S.unit_image(fake, buf=True, nchw=False)[1], S.unit_image(real, buf=True, nchw=False)[1]
        r = S.unet_logits(P, B, R0, batch_stats, update_running=False)
        z, saved = S.unet_logits(P, B, F0, batch_stats, save="input", update_running=False)
        res = torch.zeros(2, dtype=torch.int64, device=DEV)
        g = Buf.empty(N, H, W, 4, 0, DEV)
        ops.flood_mask_bce(z, r, 1.0 / (N * H * W), g, res)
        g_in = S.unet_backward(P, saved, g, input_grad=True, param_grads=False)["input"]
        out = torch.full_like(fake, NAN)
        ops.unit_image_bwd(g_in, fake, out)
    return res.cpu(), out, z, r


@pytest.mark.parametrize("batch_stats", [False, True])
def test_flood_mask_loss_module(batch_stats, monkeypatch):
    from floodgan import FloodMaskLoss
    from floodgan import segmentation as S
    from floodgan.evaluate import MaskConfusion
    net = _perturbed_module(26).to(DEV)
    net.train(not batch_stats)                             # the module's own flag is not what decides
    fake, real = _images(90)
    with torch.no_grad():                                  # centre the head, so that the target mask has both classes
        net.outc.conv.bias -= FloodMaskLoss(net, batch_stats=batch_stats).logits(real, real)[1].median()
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    loss = FloodMaskLoss(net, batch_stats=batch_stats)
    fake.requires_grad_(True)
    real.requires_grad_(True)
    value = loss(fake, real)
    assert value.dim() == 0 and value.requires_grad
    value.backward()
    assert real.grad is None and fake.grad is not None
    assert all(p.grad is None for p in net.parameters())
    res, g_hand, z, r = _by_hand(net, fake.detach(), real.detach(), batch_stats)
    assert torch.equal(fake.grad, g_hand)                                   # bit for bit
    assert float(fake.grad.abs().max()) > 0
    value = value.detach()
    assert float(value) == float(res[:1].view(torch.float32)[0])
    # the value against torch's BCE of the module's own logits and the device's own mask
    zl, rl = loss.logits(fake.detach(), real.detach())
    assert torch.equal(zl.cpu(), nchw(z, 1)) and torch.equal(rl.cpu(), nchw(r, 1))
    t = device_flood(rl)[:, None].double()
    ref = float(F.binary_cross_entropy_with_logits(zl.double().cpu(), t))
    print(f"FloodMaskLoss batch_stats {batch_stats}: {float(value)} vs {ref}; target flood fraction "
          f"{float(t.mean()):.3f}")
    assert abs(float(value) - ref) / ref < 1e-6
    assert 0.2 < float(t.mean()) < 0.8
    conf = MaskConfusion(DEV)
    conf.update(z, r)
    tp, fp, tn, fn = (int(v) for v in conf.counts.cpu())
    assert loss.agreement == (tp + tn) / t.numel() and loss.read() == (float(value), loss.agreement)
    # no gradient asked for: nothing is saved
    calls = []
    real_fn = S.unet_logits
    monkeypatch.setattr(S, "unet_logits", lambda *a, **k: (calls.append(k.get("save", False)), real_fn(*a, **k))[1])
    with torch.no_grad():
        v2 = loss(fake, real)
    v3 = loss(fake.detach(), real)
    assert calls == [False] * 4 and not v2.requires_grad and not v3.requires_grad and v2.grad_fn is None
    assert float(v2) == float(value) == float(v3)
    v4 = loss(fake, real)
    assert calls[4:] == [False, "input"] and v4.requires_grad
    monkeypatch.undo()
    # the frozen network was left alone, bit for bit, in both BatchNorm modes
    for k, v in net.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert net.training == (not batch_stats)
    if batch_stats:
        # batch statistics: the logits of two separate train-mode calls of the same network, one per image set
        twin = copy.deepcopy(net).train()
        with torch.no_grad():
            za = twin(S.unit_image(fake.detach())[0])
            rb = twin(S.unit_image(real.detach())[0])
        assert torch.equal(za, zl) and torch.equal(rb, rl)


def test_flood_mask_loss_takes_a_model_or_a_checkpoint(tmp_path):
    from floodgan import FloodMaskLoss
    from floodgan.segmentation import SegmentationModel
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(27)
        m = SegmentationModel(device=DEV, verbose=False)
    path = str(tmp_path / "seg.pth.tar")
    torch.save(m.checkpoint(0), path)
    fake, real = _images(91)
    a, b = FloodMaskLoss(m), FloodMaskLoss(path)
    assert a.seg is m.model and b.seg is not m.model
    assert float(a(fake, real)) == float(b(fake, real))


@pytest.mark.parametrize("training", [True, False])
def test_unet_input_grad_switch(training):
    """UNet.input_grad = True: stock autograd reaches the input image, in train and in eval mode"""
    from floodgan import ops
    from floodgan import segmentation as S
    from floodgan.plans import Buf
    net = _perturbed_module(28).to(DEV)
    net.train(training)
    net.input_grad = True
    ref_net = copy.deepcopy(net)
    x, t = _batch(2, 32, 32, 51)
    xd, td = x.to(DEV).requires_grad_(True), t.to(DEV)
    seen = []
    out = net(xd)
    out.register_hook(lambda g: seen.append(g.detach().clone()))
    F.binary_cross_entropy_with_logits(out, td).backward()
    assert xd.grad is not None and all(p.grad is not None for p in net.parameters())
    P, B = dict(ref_net.named_parameters()), dict(ref_net.named_buffers())
    with torch.no_grad():
        logits, saved = S.unet_logits(P, B, S.unit_image_passthrough(xd.detach())[1], training, save=True)
        g = Buf.empty(2, 32, 32, 4, 0, DEV)
        ops.pack_input(seen[0], 1, None, 0, g, 0, 2, 0)
        grads = S.unet_backward(P, saved, g, input_grad=True)
    assert torch.equal(nchw(logits, 1), out.detach().cpu())
    assert torch.equal(xd.grad.cpu(), nchw(grads["input"], 3)) and float(xd.grad.abs().max()) > 0
    worst = max((nrel(p.grad, grads[k]), k) for k, p in net.named_parameters())
    assert worst[0] < 1e-6, worst
    # the input gradient alone (frozen parameters): the lean state, the same gradient
    for p in net.parameters():
        p.requires_grad_(False)
    x2 = xd.detach().clone().requires_grad_(True)
    if training:
        net.load_state_dict(ref_net.state_dict())          # (the first train-mode call moved the running statistics)
    F.binary_cross_entropy_with_logits(net(x2), td).backward()
    assert torch.equal(x2.grad, xd.grad)


def test_default_unet_keeps_both_documented_errors():
    from floodgan.segmentation import UNet
    net = _init_module(29).to(DEV)
    assert type(net) is UNet and net.input_grad is False
    x, t = _batch(1, 16, 16, 52)
    with pytest.raises(RuntimeError, match="input image"):
        net(x.to(DEV).requires_grad_(True))
    net.eval()
    out = net(x.to(DEV))
    with pytest.raises(RuntimeError, match="eval"):
        F.binary_cross_entropy_with_logits(out, t.to(DEV)).backward()


# ------------------------------------------------------------------------------------------ the fused paired step

def _paired_batch():
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand((2, 9, 64, 64), generator=g) * 2 - 1, torch.rand((2, 3, 64, 64), generator=g) * 2 - 1
    return x.to(DEV), y.to(DEV)


def test_fused_step_default_is_unchanged():
    from floodgan.model import Model
    x, y = _paired_batch()
    out = []
    for kw in ({}, dict(flood_mask_weight=0.0, segmentation_model_path=None, flood_mask_batch_stats=False)):
        m = Model(model="PairedAttention", num_epochs=2, **kw)
        assert m.step_fn.fake_loss is None
        losses = m.step_fn(x, y)
        assert losses.shape == (4,)
        out.append((losses.cpu(), [p.detach().cpu() for p in list(m.generator.parameters())
                                   + list(m.discriminator.parameters())]))
    assert torch.equal(out[0][0], out[1][0])
    assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))


def test_fused_step_with_the_flood_mask_term(tmp_path):
    from floodgan import FloodMaskLoss
    from floodgan.model import Model
    from floodgan.segmentation import SegmentationModel
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(30)
        seg = SegmentationModel(device=DEV, verbose=False)
    path = str(tmp_path / "seg.pth.tar")
    torch.save(seg.checkpoint(0), path)
    x, y = _paired_batch()
    plain = Model(model="PairedAttention", num_epochs=2)
    m = Model(model="PairedAttention", num_epochs=2, flood_mask_weight=0.25, segmentation_model_path=path)
    for a, b in zip(plain.generator.parameters(), m.generator.parameters()):
        assert torch.equal(a, b)                           # loading the U-Net did not move the model's RNG stream
    step = m.step_fn
    term, rec = step.fake_loss, {}
    assert term.weight == 0.25 and term.loss is m.flood_mask_loss and not term.loss.batch_stats

    def spy(fake, real, g_fake, scale):
        rec.update(before=g_fake.detach().clone(), scale=scale, real=real)
        out = term(fake, real, g_fake, scale)
        rec.update(after=g_fake.detach().clone())
        return out

    spy.weight = term.weight
    step.fake_loss = spy
    losses = step(x, y)
    assert losses.shape == (5,) and rec["scale"] == 0.25 and rec["real"] is y
    ref4 = plain.step_fn(x, y)
    assert torch.equal(losses[:4], ref4)                   # the four terms ahead of the hook
    assert torch.equal(rec["before"], _l1_gradient(step.last_output, y))
    # the fifth loss and the added gradient: the stand-alone module on the recorded output
    alone = FloodMaskLoss(seg)
    fake = step.last_output.detach().clone().requires_grad_(True)
    value = alone(fake, y)
    value.backward()
    assert float(losses[4]) == 0.25 * float(value) > 0
    want = rec["before"].double() + 0.25 * fake.grad.double()
    err = (rec["after"].double() - want).abs()
    assert bool((err <= ULP * want.abs() + 1e-45).all()), float((err / want.abs().clamp_min(1e-30)).max())
    assert not torch.equal(rec["after"], rec["before"])
    # the log: the new key beside the reference's four, one entry per epoch
    key = "all_losses_flood_mask_generator_synthetic"
    assert list(m.all_losses)[4] == key and len(plain.all_losses) == 4
    m.num_epochs = 1
    m.train_loader = [(x, y, ["a", "b"])]
    m.train_paired()
    assert all(len(v) == 1 for v in m.all_losses.values()) and m.all_losses[key][0] > 0


def _l1_gradient(fake, y):
    """the L1 term's gradient as the step forms it (ops.l1 with the step's scale), before anything is added"""
    from floodgan import ops
    g = torch.empty_like(y)
    ops.l1(fake, y, 100.0, torch.empty(1, device=DEV), g, loss_scale=100.0)
    return g
