"""Training the flood-segmentation U-Net on the device (floodgan.segmentation: fg_bce_logits, fg_maxpool2_bwd,
unet_backward, SegStep, SegmentationModel.train_model) against fp64 torch and the CPU oracle of the step
(tests/seg_train_oracle.py, pinned to the reference's own train_model by tests/test_seg_train_oracle_golden.py).

Gradients are compared teacher-forced: the fp64 oracle takes the HIP path's ReLU decisions and max-pool choices, and
every decision that differs must sit within rounding of its kink (KINK).  Free-running, the reference differs from
itself by up to 7e-3 in single tensors (one flipped decision moves a whole network's gradients), so no free-running
gradient comparison is made."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_train_oracle as SO
from test_gpu_northstar import KINK, _update_agreement
from test_gpu_parity import DEV, KTOL, MATHS, NTOL, buf_from, conv_math, nchw, nrel  # noqa: F401  (conv_math: fixture)
from test_seg_train_oracle_golden import EPOCHS, NUM_EPOCHS, checksum, load_gold, synth_batches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from floodgan import _lib as L
    L.check(L.load().fg_device_ok(), "device_ok")
    torch.set_num_threads(min(16, max(1, len(os.sched_getaffinity(0)))))


# ------------------------------------------------------------------------------------------ kernels

def test_bce_logits_vs_fp64():
    from floodgan import ops
    from floodgan.plans import Buf
    N, H, W = 2, 40, 48
    g = torch.Generator().manual_seed(11)
    z = torch.randn((N, 1, H, W), generator=g) * 3
    special = [0.0, 1e-3, -1e-3, 20.0, -20.0, 90.0, -90.0]
    tv = torch.tensor([0.0, 1.0, 0.3])
    t = tv[torch.randint(0, 3, (N, 1, H, W), generator=g)]
    for i, s in enumerate(special):                      # every special logit against every target value
        for j in range(3):
            z[i % N, 0, 3 + i, 5 + j] = s
            t[i % N, 0, 3 + i, 5 + j] = tv[j]
    logits = buf_from(z, 1, "constant", 4)
    logits.nhwc()[..., 1:] = 7.0                         # only channel 0 is read
    gscale = 1.0 / z.numel()
    td = t.to(DEV)
    runs = []
    for _ in range(2):
        grad = Buf(torch.full(((N * (H + 2) * (W + 2)) * 4,), float("nan"), device=DEV), N, H, W, 4, 1)
        res = torch.zeros(2, dtype=torch.int64, device=DEV)
        ops.bce_logits(logits, td, gscale, grad, res[:1].view(torch.float32), res[1:])
        runs.append((grad.nhwc().cpu(), res.cpu()))
    (gr, res), (gr2, res2) = runs
    assert torch.equal(gr, gr2) and torch.equal(res, res2)              # deterministic: bit-identical
    z64, t64 = z.double(), t.double()
    loss_ref = float(F.binary_cross_entropy_with_logits(z64, t64))
    g_ref = (torch.sigmoid(z64) - t64) * gscale
    correct_ref = int(((torch.sigmoid(z64) > 0.5) == (t64 > 0.5)).sum())
    loss = float(res[:1].view(torch.float32)[0])
    e_loss, e_grad = abs(loss - loss_ref) / loss_ref, nrel(gr[:, 1:-1, 1:-1, 0], g_ref[:, 0])
    print(f"bce_logits: loss {loss} vs {loss_ref} (rel {e_loss:.2e}); gradient nrel {e_grad:.2e}; "
          f"correct {int(res[1])} vs {correct_ref}")
    assert e_loss < 1e-6
    assert e_grad < 1e-6
    assert int(res[1]) == correct_ref
    assert not torch.isnan(gr).any()
    assert float(gr[..., 1:].abs().max()) == 0.0                       # padded channels
    border = gr.clone()
    border[:, 1:-1, 1:-1] = 0
    assert float(border.abs().max()) == 0.0


@pytest.mark.parametrize("N,H,W,pad", [(1, 516, 512, 0), (2, 37, 45, 1)])
def test_bce_logits_grid_stride_and_second_quad(N, H, W, pad):
    """fg_bce_logits where its loops go round again: 516 x 512 is 264192 pixels, more than the 1024 blocks x 256
    threads the launch is capped at, so the grid-stride loop takes a second iteration for the last 2048 of them (the
    workload's 1024^2 takes four); the gradient buffer has 8 channels, so the channel-quad loop writes a second
    quad.  The second shape has a border on both buffers.  Same assertions as test_bce_logits_vs_fp64"""
    from floodgan import ops
    from floodgan.plans import Buf
    g = torch.Generator().manual_seed(12 + pad)
    z = torch.randn((N, 1, H, W), generator=g) * 3
    special = [0.0, 1e-3, -1e-3, 20.0, -20.0, 90.0, -90.0]
    tv = torch.tensor([0.0, 1.0, 0.3])
    t = tv[torch.randint(0, 3, (N, 1, H, W), generator=g)]
    for i, s in enumerate(special):                      # every special logit against every target value, at the
        for j in range(3):                               # start of the pixel range and inside its last 2048
            for y0 in (3, H - len(special)):
                z[i % N, 0, y0 + i, 5 + j] = s
                t[i % N, 0, y0 + i, 5 + j] = tv[j]
    if pad == 0:
        assert N * H * W > 1024 * 256
    logits = buf_from(z, pad, "constant", 4)
    logits.nhwc()[..., 1:] = 7.0                         # only channel 0 is read
    gscale = 1.0 / z.numel()
    td = t.to(DEV)
    runs = []
    for _ in range(2):
        grad = Buf(torch.full(((N * (H + 2 * pad) * (W + 2 * pad)) * 8,), float("nan"), device=DEV), N, H, W, 8, pad)
        res = torch.zeros(2, dtype=torch.int64, device=DEV)
        ops.bce_logits(logits, td, gscale, grad, res[:1].view(torch.float32), res[1:])
        runs.append((grad.nhwc().cpu(), res.cpu()))
    (gr, res), (gr2, res2) = runs
    assert torch.equal(gr, gr2) and torch.equal(res, res2)              # deterministic: bit-identical
    z64, t64 = z.double(), t.double()
    loss_ref = float(F.binary_cross_entropy_with_logits(z64, t64))
    g_ref = (torch.sigmoid(z64) - t64) * gscale
    correct_ref = int(((torch.sigmoid(z64) > 0.5) == (t64 > 0.5)).sum())
    loss = float(res[:1].view(torch.float32)[0])
    inner = gr[:, pad:pad + H, pad:pad + W]
    e_loss, e_grad = abs(loss - loss_ref) / loss_ref, nrel(inner[..., 0], g_ref[:, 0])
    print(f"bce_logits {N}x{H}x{W} pad {pad}: loss {loss} vs {loss_ref} (rel {e_loss:.2e}); gradient nrel "
          f"{e_grad:.2e}; correct {int(res[1])} vs {correct_ref}")
    assert e_loss < 1e-6
    assert e_grad < 1e-6
    assert int(res[1]) == correct_ref
    assert not torch.isnan(gr).any()                                    # every pixel of the padded extent written
    assert float(gr[..., 1:].abs().max()) == 0.0                       # padded channels, both quads
    border = gr.clone()
    border[:, pad:pad + H, pad:pad + W] = 0
    assert float(border.abs().max()) == 0.0


def _pool_source(N, C, H, W, seed):
    """post-ReLU values with every kind of window: all zero, four and two equal positive maxima, and a strict
    maximum in each of the four positions (in every channel and image), random post-ReLU windows elsewhere"""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn((N, C, H, W), generator=g))
    x[:, :, 0:2, 0:2] = 0.0
    x[:, :, 0:2, 2:4] = 1.5
    x[:, :, 0:2, 4:6] = 0.5
    x[:, :, 0, 5] = 2.0
    x[:, :, 1, 4] = 2.0                                   # positions 1 and 2 tie: the first (0, 1) wins
    for p in range(4):
        x[:, :, 2:4, 2 * p:2 * p + 2] = 0.25
        x[:, :, 2 + p // 2, 2 * p + p % 2] = 3.0
    return x


@pytest.mark.parametrize("C", [64, 4])
def test_maxpool2_bwd_bit_exact(C):
    from floodgan import ops
    from floodgan.plans import Buf
    N, H, W = 2, 8, 12
    x = _pool_source(N, C, H, W, 5 + C)
    gy = torch.randn((N, C, H // 2, W // 2), generator=torch.Generator().manual_seed(6))
    xr = x.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.max_pool2d(xr, 2), xr, gy)
    src, gp = buf_from(x, 0, "constant"), buf_from(gy, 1, "constant")
    dst = Buf(torch.full((N * (H + 2) * (W + 2) * C,), float("nan"), device=DEV), N, H, W, C, 1)
    choice = torch.full((N, H // 2, W // 2, C), 9, dtype=torch.uint8, device=DEV)
    ops.maxpool2_bwd(src, gp, dst, choice)
    got = nchw(dst)
    assert torch.equal(got, ref)                                        # every interior element written, bit-exact
    first = SO.first_max(x)
    assert torch.equal(choice.permute(0, 3, 1, 2).cpu().long(), first)
    assert int(first[0, 0, 0, 0]) == 0 and int(first[0, 0, 0, 1]) == 0 and int(first[0, 0, 0, 2]) == 1
    assert [int(first[0, 0, 1, p]) for p in range(4)] == [0, 1, 2, 3]
    # the forward pools the same values
    pooled = Buf.zeros(N, H // 2, W // 2, C, 0, DEV)
    ops.maxpool2(src, pooled)
    assert torch.equal(nchw(pooled), F.max_pool2d(x, 2))


def _maxpool2_bwd_case(x, spad, dpad, gpad, seed):
    """fg_maxpool2_bwd of the source x (NCHW, any H, W >= 2) into a NaN-filled destination, bit-exact against
    autograd's max_pool2d gradient (zero in an odd last row / column) and against SO.first_max"""
    from floodgan import ops
    from floodgan.plans import Buf
    N, C, H, W = x.shape
    gy = torch.randn((N, C, H // 2, W // 2), generator=torch.Generator().manual_seed(seed))
    xr = x.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.max_pool2d(xr, 2), xr, gy)
    src, gp = buf_from(x, spad, "constant"), buf_from(gy, gpad, "constant")
    dst = Buf(torch.full((N * (H + 2 * dpad) * (W + 2 * dpad) * C,), float("nan"), device=DEV), N, H, W, C, dpad)
    choice = torch.full((N, H // 2, W // 2, C), 9, dtype=torch.uint8, device=DEV)
    ops.maxpool2_bwd(src, gp, dst, choice)
    got = nchw(dst)
    assert torch.equal(got, ref)                         # every interior element written, bit-exact
    if H % 2:
        assert float(got[:, :, -1].abs().max()) == 0.0   # outside every window: exactly zero, not left NaN
    if W % 2:
        assert float(got[:, :, :, -1].abs().max()) == 0.0
    full = dst.nhwc().cpu()
    full[:, dpad:dpad + H, dpad:dpad + W] = float("nan")
    assert bool(torch.isnan(full).all())                 # the destination's border is not touched
    first = SO.first_max(x[:, :, :H // 2 * 2, :W // 2 * 2])
    assert torch.equal(choice.permute(0, 3, 1, 2).cpu().long(), first)
    return first


@pytest.mark.parametrize("H,W,spad,dpad", [(7, 9, 0, 1), (7, 9, 1, 0), (3, 2, 0, 1), (3, 2, 1, 0)])
def test_maxpool2_bwd_odd_sizes_and_pads(H, W, spad, dpad):
    """the kernel's !full branch: an odd last row / column of the source lies outside every pooled window and its
    gradient is written as zero; source and destination with different borders (their strides differ)"""
    if W >= 8:
        x = _pool_source(2, 8, H, W, 7)                  # its ties and strict maxima sit in rows 0..3, columns 0..7
    else:
        x = torch.relu(torch.randn((2, 8, H, W), generator=torch.Generator().manual_seed(8)))
        x[:, :4, 0:2, 0:2] = 1.5                         # a four-way tie in half of the channels: position 0 wins
    first = _maxpool2_bwd_case(x, spad, dpad, 1 - dpad, 9)
    if W >= 8:
        assert [int(first[0, 0, 1, p]) for p in range(4)] == [0, 1, 2, 3]
    else:
        assert int(first[0, 0, 0, 0]) == 0


def test_maxpool2_bwd_grid_stride():
    """1 x 256 x 258 x 256: 129 * 128 * 64 = 1,056,768 (window, channel quad) items, more than the 4096 blocks x 256
    threads the launch is capped at -- the grid-stride loop takes a second iteration (the workload's 1024^2 level-1
    pool has 4.2 M items)"""
    N, C, H, W = 1, 256, 258, 256
    assert N * (H // 2) * (W // 2) * (C // 4) > 4096 * 256
    x = _pool_source(N, C, H, W, 10)
    x[:, :, -2:] = x[:, :, 0:2]                          # the same ties in the windows of the second iteration
    first = _maxpool2_bwd_case(x, 0, 0, 0, 11)
    assert int(first[0, 0, 0, 0]) == 0 and int(first[0, 0, 0, 1]) == 0 and int(first[0, 0, 0, 2]) == 1
    assert torch.equal(first[:, :, -1], first[:, :, 0])


@pytest.mark.parametrize("N,H,W", [(2, 5, 7), (1, 96, 96)])
def test_conv1x1_head_one_output_in_four_channels(N, H, W):
    """fg_conv1x1_dgrad / fg_conv1x1_wgrad as the segmentation head calls them: n_out = 1 with a 4-channel gradient
    buffer (test_conv1x1_head has 16 channels and n_out 3 .. 16).  Channels 1..3 of the gradient are NaN: never
    read; the weight gradient written, then accumulated"""
    from floodgan import ops
    from floodgan.plans import Buf
    g = torch.Generator().manual_seed(33)
    x = torch.randn((N, 64, H, W), dtype=torch.float64, generator=g)
    w = (torch.randn((1, 64, 1, 1), dtype=torch.float64, generator=g) * 0.1).requires_grad_(True)
    b = torch.randn((1,), dtype=torch.float64, generator=g).requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    y = F.conv2d(xr, w, b)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    gx_ref, gw_ref, gb_ref = torch.autograd.grad(y, (xr, w, b), gy)
    X = buf_from(x, 0, "constant")
    wd = w.detach().float().to(DEV)
    GY = buf_from(gy, 0, "constant", c_alloc=4)
    GY.nhwc()[..., 1:] = float("nan")
    GX = Buf(torch.full((N * H * W * 64,), float("nan"), device=DEV), N, H, W, 64, 0)
    ops.conv1x1_dgrad(GY, wd, 1, GX)
    dw = torch.full(w.shape, 3.0, device=DEV)
    db = torch.full((1,), -2.0, device=DEV)
    ops.conv1x1_wgrad(GY, X, 1, dw, db)
    torch.cuda.synchronize()
    e = dict(dgrad=nrel(nchw(GX), gx_ref), wgrad=nrel(dw, gw_ref), bgrad=nrel(db, gb_ref))
    ops.conv1x1_wgrad(GY, X, 1, dw, db, accumulate=True)
    torch.cuda.synchronize()
    e.update(wgrad_acc=nrel(dw, 2 * gw_ref), bgrad_acc=nrel(db, 2 * gb_ref))
    print(f"conv1x1 head n_out 1 in 4 channels, {N}x{H}x{W}:", e)
    assert max(e.values()) < KTOL, e


@pytest.mark.parametrize("conv_math", MATHS, indirect=True)
def test_head_forward_one_output_in_four_channels(conv_math, report):
    """the OutConv forward as unet_logits runs it: a 1x1 conv with one output on the conv engine into the 4-channel
    logits buffer, in every conv math; channels 1..3 are not written"""
    from floodgan import ops, pix2pix as P2P
    from floodgan.plans import Buf
    N, H, W = 2, 6, 10
    g = torch.Generator().manual_seed(34)
    x = torch.randn((N, 64, H, W), dtype=torch.float64, generator=g)
    w = torch.randn((1, 64, 1, 1), dtype=torch.float64, generator=g) * 0.1
    b = torch.randn((1,), dtype=torch.float64, generator=g)
    ref = F.conv2d(x, w, b)
    P = {"outc.conv.weight": w.float().to(DEV), "outc.conv.bias": b.float().to(DEV)}
    logits = Buf(torch.full((N * H * W * 4,), float("nan"), device=DEV), N, H, W, 4, 0)
    P2P._conv_nb(P, "outc.conv", buf_from(x, 0, "constant"), 0, 1, 1, logits)
    kernel = ops.LAST_CONV_KERNEL
    out = logits.nhwc().cpu()
    e = nrel(out[..., 0], ref[:, 0])
    print(f"segmentation head forward [{conv_math}]: nrel {e:.2e} ({kernel})")
    report("seg_head_forward", math=conv_math, nrel=e, kernel=kernel)
    # one output: below the pipelined kernel's 33 (fgc::f3_config), so f16x3 runs its register-staged kernel
    assert kernel == {"fp32": "conv_fwd"}.get(conv_math, "conv_fwd_x6")
    assert e < KTOL
    assert bool(torch.isnan(out[..., 1:]).all())


@pytest.mark.parametrize("shape", [(2, 128, 6, 10), (1, 1024, 2, 2)])
def test_convT2_backward_vs_fp64(shape):
    """ConvTranspose2d(k=2, s=2, p=0) backward alone at the narrowest and the widest level"""
    from floodgan import layers
    from floodgan import segmentation as S
    N, Cin, H, W = shape
    g = torch.Generator().manual_seed(Cin)
    x = torch.randn(shape, generator=g)
    w = torch.randn((Cin, Cin // 2, 2, 2), generator=g) * 0.05
    b = torch.randn((Cin // 2,), generator=g)
    gy = torch.randn((N, Cin // 2, 2 * H, 2 * W), generator=g)
    P = {"up.weight": w.to(DEV), "up.bias": b.to(DEV)}
    G = layers.Grads(P)
    g_x = S._convT2_bwd(P, G, "up", buf_from(x, 1, "constant"), buf_from(gy, 0, "constant"))
    rx, rw, rb = SO.convT2_grads(x.double(), w.double(), b.double(), gy.double())
    e = dict(input=nrel(nchw(g_x), rx), weight=nrel(G.out["up.weight"], rw), bias=nrel(G.out["up.bias"], rb))
    print("convT2 backward", shape, e)
    assert max(e.values()) < 1e-4, e


# ------------------------------------------------------------------------------------------ whole backward

def _init_module(seed):
    from floodgan.segmentation import UNet, initialise_weights
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return UNet().apply(initialise_weights)


def _batch(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((N, 3, H, W), generator=g), (torch.rand((N, 1, H, W), generator=g) > 0.6).float()


def _hip_grads(net, x, t):
    """executor-level forward + BCE + backward: (loss, correct, logits NCHW host, grads, oracle Decisions)"""
    from floodgan import ops
    from floodgan import segmentation as S
    from floodgan.plans import Buf
    P, B = dict(net.named_parameters()), dict(net.named_buffers())
    N, _, H, W = x.shape
    with torch.no_grad():
        logits, saved = S.unet_logits(P, B, S.unit_image_passthrough(x.to(DEV))[1], True, save=True)
        res = torch.zeros(2, dtype=torch.int64, device=DEV)
        g = Buf.empty(N, H, W, 4, 0, DEV)
        ops.bce_logits(logits, t.to(DEV), 1.0 / t.numel(), g, res[:1].view(torch.float32), res[1:])
        choices = {}
        grads = S.unet_backward(P, saved, g, choices=choices)
    dec = SO.Decisions(relu=S.unet_decisions(saved), pool={k: v.cpu() for k, v in choices.items()})
    res = res.cpu()
    return float(res[:1].view(torch.float32)[0]), int(res[1]), nchw(logits, 1), grads, dec


def _logit_kinks(dec, logits_hip, logits_ref):
    """log the mask decisions (logit > 0) that differ like the activation kinks; returns their number"""
    ref = logits_ref.double()
    dis = (logits_hip.double() > 0) != (ref > 0)
    n = int(dis.sum())
    rms = float(ref.pow(2).mean().sqrt()) or 1.0
    dec.log.append(("mask", "logits", n, float(ref[dis].abs().max()) / rms if n else 0.0))
    return n


@pytest.mark.parametrize("shape", [(1, 32, 32), (2, 32, 48), (3, 48, 32)])
def test_unet_backward_teacher_forced(shape, report):
    N, H, W = shape
    cpu = _init_module(21)
    net = copy.deepcopy(cpu).to(DEV)
    x, t = _batch(N, H, W, 31)
    loss, correct, logits, grads, dec = _hip_grads(net, x, t)
    st = SO.SegStepOracle(cpu, torch.float64)
    loss_ref, acc_ref, logits_ref, ref = st.step(x, t, dec, update=False)
    rows = sorted(((k, nrel(grads[k], ref[k])) for k in ref), key=lambda r: -r[1])
    run = [(k, nrel(v, st.B[k])) for k, v in net.named_buffers() if v.is_floating_point()]
    n_mask = _logit_kinks(dec, logits, logits_ref)
    print(f"unet backward {shape}: worst gradients {rows[:3]}; {dec.differing()} decisions differ, worst kink "
          f"{dec.worst():.2e}; loss rel {abs(loss - loss_ref) / loss_ref:.2e}; worst running stat "
          f"{max(run, key=lambda r: r[1])}")
    report("seg_unet_backward_teacher_forced", shape=list(shape), worst_grad=rows[0], worst_kink=dec.worst(),
           decisions_differing=dec.differing(), loss_rel=abs(loss - loss_ref) / loss_ref,
           worst_running_stat=max(run, key=lambda r: r[1]))
    assert set(grads) == set(ref)
    assert dec.worst() < KINK, [r for r in dec.log if r[2]]
    assert rows[0][1] < 1e-4, rows[:5]
    assert max(r for _, r in run) < 1e-5, max(run, key=lambda r: r[1])
    assert abs(loss - loss_ref) / loss_ref < 1e-5
    assert abs(correct - round(acc_ref * t.numel())) <= n_mask
    for k, v in net.named_buffers():
        if not v.is_floating_point():
            assert int(v) == int(st.B[k]) == 1, k


def test_seg_step_two_iterations_teacher_forced(report):
    """two fused SegStep iterations; before each, the fp64 oracle continues from the HIP state (parameters, BatchNorm
    buffers, Adam moments)"""
    from floodgan.segmentation import SegmentationModel, SegStep
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(22)
        m = SegmentationModel(train=True, device=DEV, verbose=False)
    step = m.step_fn
    step.record_decisions = True
    m.model.train()
    for it in range(2):
        x, t = _batch(2, 32, 48, 40 + it)
        st = SO.SegStepOracle(m.model, torch.float64)
        if it:
            st.load_optimizer(m.optimizer.state_dict())
        P0 = {k: p.detach().clone() for k, p in m.model.named_parameters()}
        loss, acc = SegStep.read(step(x.to(DEV), t.to(DEV)), t.numel())
        d = step.decisions
        dec = SO.Decisions(relu=d["relu"], pool=d["pool"])
        loss_ref, acc_ref, logits_ref, ref = st.step(x, t, dec)
        n_mask = _logit_kinks(dec, d["logits"], logits_ref)
        rows, bad = [], []
        for k, p in m.model.named_parameters():
            ge = nrel(p.grad, ref[k])
            agree, uerr, frac, perr = _update_agreement(P0[k], p, st.P[k], p.grad, ref[k], st.exp_avg(k))
            rows.append((k, ge, agree, uerr, frac, perr))
            if ge > 1e-4 or agree < 1.0 or uerr > NTOL:
                bad.append(rows[-1])
        run = [(k, nrel(v, st.B[k])) for k, v in m.model.named_buffers() if v.is_floating_point()]
        lrel = abs(loss - loss_ref) / loss_ref
        print(f"SegStep it {it}: loss {loss} (rel {lrel:.2e}), accuracy {acc} vs {acc_ref}; worst gradient "
              f"{max(rows, key=lambda r: r[1])[:2]}; min agreement {min(r[2] for r in rows)}; worst decided update "
              f"{max(rows, key=lambda r: r[3])[0::3]}; min decided {min(r[4] for r in rows):.3f}; "
              f"{dec.differing()} decisions differ, worst kink {dec.worst():.2e}")
        report("seg_step_teacher_forced", it=it, loss_rel=lrel, worst_grad=max(rows, key=lambda r: r[1])[:2],
               min_agree=min(r[2] for r in rows), worst_update=max(rows, key=lambda r: r[3])[0::3],
               decisions_differing=dec.differing(), worst_kink=dec.worst(), bad=bad)
        assert dec.worst() < KINK, [r for r in dec.log if r[2]]
        assert not bad, bad
        assert max(r for _, r in run) < 1e-5
        assert lrel < 1e-5
        assert abs(acc - acc_ref) * t.numel() <= n_mask + 1e-6, (acc, acc_ref, n_mask)


# ------------------------------------------------------------------------------------------ train_model vs the golden

class _Done(Exception):
    pass


class _Loader:
    def __init__(self, batches, epochs):
        self.batches, self.left = batches, epochs

    def __iter__(self):
        if self.left == 0:
            raise _Done
        self.left -= 1
        return iter([(x, t, ["synthetic"] * x.shape[0]) for x, t in self.batches])


def _state_errors(gold, prefix, state):
    """worst |difference| of the checksum sums (sum, abs-sum) relative to the abs-sum, over the tensors"""
    worst = 0.0
    for name, v in state.items():
        ref, mine = gold[f"{prefix}/{name}"], checksum(v.cpu())
        scale = max(abs(ref[1]), 1e-12)
        worst = max(worst, abs(mine[0] - ref[0]) / scale, abs(mine[1] - ref[1]) / scale)
    return worst


def _reference_envelope(gold, sigma=1e-6, trials=2):
    """how far the reference algorithm (the fp32 oracle) itself lands from the golden run when its inputs carry
    `sigma` relative noise: per epoch (losses, accuracies, state checksums)"""
    from test_seg_train_oracle_golden import init_module
    batches = synth_batches()
    env = [[0.0, 0.0, 0.0] for _ in range(EPOCHS)]
    for trial in range(1, trials + 1):
        st = SO.SegStepOracle(init_module(), torch.float32, num_epochs=NUM_EPOCHS)
        for epoch in range(EPOCHS):
            ls, ac = [], []
            for b, (x, t) in enumerate(batches):
                noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(trial * 100 + epoch * 10 + b))
                loss, acc, _, _ = st.step(x * (1 + sigma * noise), t)
                ls.append(loss)
                ac.append(acc)
            st.sched.step()
            e = (float((np.abs(np.array(ls) - gold["losses"][epoch]) / gold["losses"][epoch]).max()),
                 float(np.abs(np.array(ac) - gold["accuracies"][epoch]).max()),
                 _state_errors(gold, f"epoch{epoch + 1}", st.state_dict()))
            env[epoch] = [max(a, b) for a, b in zip(env[epoch], e)]
    return env


def test_train_model_vs_reference_golden(report):
    """SegmentationModel.train_model over the golden's two epochs (the reference's construction under
    torch.manual_seed(5), its synthetic batches) vs the numbers the reference's own train_model recorded, inside the
    reference's own envelope under 1e-6 input noise"""
    from floodgan.segmentation import SegmentationModel
    gold = load_gold()
    env = _reference_envelope(gold)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5)
        m = SegmentationModel(train=True, num_epochs=NUM_EPOCHS, device=DEV, verbose=False)
    m.train_loader = _Loader(synth_batches(), EPOCHS)
    recorded = []
    orig = m.save_results

    def _record(epoch, losses, accuracies, t0):
        recorded.append((list(losses), list(accuracies), m.optimizer.param_groups[0]["lr"],
                         {k: v.detach().clone() for k, v in m.model.state_dict().items()}))
        return orig(epoch, losses, accuracies, t0)

    m.save_results = _record
    lr0 = m.optimizer.param_groups[0]["lr"]
    with pytest.raises(_Done):
        m.train_model()
    assert len(recorded) == EPOCHS
    assert abs(lr0 - gold["lr"][0]) < 1e-12 and abs(recorded[0][2] - gold["lr"][1]) < 1e-12
    for epoch, (losses, accs, _, state) in enumerate(recorded):
        lrel = np.abs(np.array(losses) - gold["losses"][epoch]) / gold["losses"][epoch]
        aerr = np.abs(np.array(accs) - gold["accuracies"][epoch])
        serr = _state_errors(gold, f"epoch{epoch + 1}", state)
        print(f"train_model epoch {epoch + 1}: loss rel {lrel.tolist()}, accuracy error {aerr.tolist()}, state "
              f"checksum error {serr:.2e}; reference envelope {env[epoch]}")
        report("seg_train_model_vs_reference_golden", epoch=epoch + 1, loss_rel=lrel.tolist(), acc_err=aerr.tolist(),
               state_err=serr, reference_envelope=env[epoch])
        if epoch == 0:       # the first batch's loss and accuracy are evaluated before any update
            assert lrel[0] < 1e-5, lrel
            assert accs[0] == gold["accuracies"][0, 0]
        assert lrel.max() < max(NTOL, 2 * env[epoch][0]), (lrel, env[epoch])
        assert aerr.max() < max(NTOL, 2 * env[epoch][1]), (aerr, env[epoch])
        assert serr < max(NTOL, 2 * env[epoch][2]), (serr, env[epoch])
    assert np.allclose(m.all_losses, gold["all_losses"], rtol=max(NTOL, 2 * max(e[0] for e in env)))
    assert m.current_epoch == EPOCHS


# ------------------------------------------------------------------------------------------ drop-in autograd path

def test_drop_in_autograd_path(monkeypatch):
    from floodgan import ops
    from floodgan import segmentation as S
    from floodgan.plans import Buf
    net = _init_module(23).to(DEV)
    ref_net = copy.deepcopy(net)
    x, t = _batch(2, 32, 32, 50)
    xd, td = x.to(DEV), t.to(DEV)
    seen = []
    out = net(xd)
    assert out.requires_grad and out.shape == (2, 1, 32, 32)
    out.register_hook(lambda g: seen.append(g.detach().clone()))
    F.binary_cross_entropy_with_logits(out, td).backward()
    assert len(seen) == 1 and all(p.grad is not None for p in net.parameters())
    # the same gradient through the executor
    P, B = dict(ref_net.named_parameters()), dict(ref_net.named_buffers())
    with torch.no_grad():
        logits, saved = S.unet_logits(P, B, S.unit_image_passthrough(xd)[1], True, save=True)
        g = Buf.empty(2, 32, 32, 4, 0, DEV)
        ops.pack_input(seen[0], 1, None, 0, g, 0, 2, 0)
        grads = S.unet_backward(P, saved, g)
    assert torch.equal(nchw(logits, 1), out.detach().cpu())
    worst = max((nrel(p.grad, grads[k]), k) for k, p in net.named_parameters())
    print("drop-in autograd vs unet_backward: worst", worst)
    assert worst[0] < 1e-6, worst
    # a stock optimizer step, then evaluation under no_grad: nothing is saved
    torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.5, 0.999)).step()
    calls = []
    real = S.unet_logits
    monkeypatch.setattr(S, "unet_logits", lambda *a, **k: (calls.append(k.get("save", False)), real(*a, **k))[1])
    with torch.no_grad():
        out2 = net(xd)
    assert calls == [False] and not out2.requires_grad and out2.grad_fn is None
    assert torch.isfinite(out2).all() and not torch.equal(out2, out.detach())
    # eval mode with grad mode on: nothing is saved either, and the backward raises the documented error
    net.eval()
    out3 = net(xd)
    assert calls == [False, False] and out3.requires_grad
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="eval"):
        F.binary_cross_entropy_with_logits(out3, td).backward()
    net.train()
    # so does a gradient of the input image
    with pytest.raises(RuntimeError, match="input image"):
        net(xd.clone().requires_grad_(True))
    # a parameter updated in place between forward and backward is caught by autograd's version check
    out4 = net(xd)
    with torch.no_grad():
        net.outc.conv.weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        F.binary_cross_entropy_with_logits(out4, td).backward()


def test_maxpool2_bwd_choice_is_validated():
    from floodgan import ops
    from floodgan.plans import Buf
    src, gp, dst = Buf.zeros(1, 4, 4, 8, 0, DEV), Buf.zeros(1, 2, 2, 8, 0, DEV), Buf.zeros(1, 4, 4, 8, 0, DEV)
    for bad in (torch.zeros((1, 2, 2, 4), dtype=torch.uint8, device=DEV),        # fewer channels than the source
                torch.zeros((1, 2, 2, 8), dtype=torch.int32, device=DEV),
                torch.zeros((1, 8, 2, 2), dtype=torch.uint8, device=DEV).permute(0, 2, 3, 1)):
        with pytest.raises(RuntimeError, match="choice must be"):
            ops.maxpool2_bwd(src, gp, dst, bad)
    ops.maxpool2_bwd(src, gp, dst, torch.zeros((1, 2, 2, 8), dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("use_test_data", [False, True])
def test_calculate_metrics_vs_mask_confusion(use_test_data, tmp_path):
    """SegmentationModel.calculate_metrics over a synthetic loader: the table MaskConfusion gives for the counts of
    the model's own flood masks (training-mode BatchNorm, as the reference evaluates) against the true masks"""
    from floodgan.evaluate import MaskConfusion
    from floodgan.segmentation import SegmentationModel
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(24)
        m = SegmentationModel(device=DEV, verbose=False, use_test_data=use_test_data)
    batches = [_batch(2, 32, 48, 60) + (["a", "b"],), _batch(1, 32, 32, 61) + (["c"],)]
    other = [_batch(1, 32, 32, 62) + (["d"],)]
    m.val_loader, m.test_loader = (other, batches) if use_test_data else (batches, other)
    probe = copy.deepcopy(m.model)
    counts = torch.zeros(4, dtype=torch.int64)
    for x, t, _ in batches:
        with torch.no_grad():
            pred = probe(x.to(DEV)).cpu() > 0                      # sigmoid(z) > 0.5
        true = t > 0.5
        counts += torch.tensor([int((pred & true).sum()), int((pred & ~true).sum()), int((~pred & ~true).sum()),
                                int((~pred & true).sum())])
    ref = MaskConfusion(DEV)
    ref.counts.copy_(counts)
    expected = ref.compute()
    m.data_path = str(tmp_path)
    df = m.calculate_metrics(use_test_data)
    assert list(df.columns) == list(expected) and len(df) == 1
    assert int(counts.sum()) == 2 * 32 * 48 + 32 * 32 and 0 < expected["Accuracy"] < 1
    for k, v in expected.items():
        assert float(df[k].iloc[0]) == v, (k, float(df[k].iloc[0]), v)
    (written,) = os.listdir(tmp_path / "metrics")
    assert written.startswith("SegmentationModel_epoch0_usaData_date") and written.endswith(".csv")
