"""The flood-segmentation U-Net the evaluation scores generator outputs with:
drop-in modules and a native forward / backward executor on the layer kit (floodgan.layers).

Reference: models/model_architectures.py:508-587 (UNet, DoubleConv, Down, Up, OutConv; milesial
style, bilinear=False), models/segmentation_model.py:19-72 (SegmentationModel: construction,
initialise_weights, checkpoint format).  The reference evaluates it without ever calling .eval()
(models/model.py:380-400, models/group.py:136-163): its BatchNorm layers run in training mode --
batch statistics, running statistics updated -- and so does this executor unless the module is put in
eval mode.

Layout.  Encoder level k (x1..x5 = 64..1024 channels at H / 2^(k-1)) is a DoubleConv (3x3 conv, no bias
-> BatchNorm -> ReLU, twice) whose last BatchNorm pass writes the level output twice: as the next
level's max-pool source and, for x1..x4, into the first channel half of the matching decoder level's
cat buffer (torch.cat([x2, x1], 1) of Up.forward, :579).  Each decoder level's ConvTranspose2d(2, 2)
(one tap per output phase: four 1x1 GEMMs, bias fused) writes straight into the second half.  The
1x1 OutConv produces the logits; the flood mask is sigmoid(logits) > 0.5.

Training (models/segmentation_model.py:250-277).  unet_logits(save=True) keeps, per DoubleConv, its input, both
conv outputs with their batch statistics and the first activation, and per level the activated output; under
torch.no_grad() nothing is kept.  unet_backward walks the graph in reverse: OutConv (1x1, fp32 FMA kernels), then per
decoder level the DoubleConv (BatchNorm backward through the batch statistics with the ReLU folded in, 3x3 weight and
input gradients on the conv engine) whose input gradient -- the gradient of the cat -- is produced as its two channel
halves in one launch: the skip half waits for the encoder, the other half goes through the ConvTranspose2d(2, 2)
backward (input gradient: one k=2, stride-2 GEMM with K = 4 C_out; weight gradient; bias = channel sums).  Each
encoder level's last BatchNorm backward sums its two consumers' gradients: the max-pool's (fg_maxpool2_bwd: first
maximum of the window, ATen's tie rule) and the skip's.
"""
import time

import numpy as np
import torch
import torch.nn as nn

from . import ops
from . import plans as PL
from ._lib import FG_ACT_RELU, FG_PAD_ZERO, require_device
from .layers import Grads, bn_stats_for, conv_fwd, convT_bwd, convT_fwd, decided, dgrad_s1, wgrad_conv
from .plans import Buf, Slice

ENC = [64, 128, 256, 512, 1024]


def _dc(prefix):
    """(conv1, bn1, conv2, bn2) parameter prefixes of a DoubleConv at `prefix`"""
    return [f"{prefix}.double_conv.{i}" for i in (0, 1, 3, 4)]


def layer_names():
    """the executor's view of the state_dict: DoubleConvs by level, the up convs, the head"""
    enc = [_dc("inc")] + [_dc(f"down{k}.maxpool_conv.1") for k in range(1, 5)]
    dec = [(f"up{k}.up", _dc(f"up{k}.conv")) for k in range(1, 5)]
    return enc, dec, "outc.conv"


def check_input_size(H, W):
    if H % 16 or W % 16:
        raise RuntimeError(f"segmentation UNet: H, W must be multiples of 16 (got {H}x{W}); the reference pads the "
                           "up path for other sizes (models/model_architectures.py:575-578), which this executor "
                           "does not implement")


def _stats(B, name, src, training, update_running):
    """layers.bn_stats_for, or -- a frozen network evaluated as the reference evaluates it -- the batch statistics
    with the running statistics and num_batches_tracked left alone"""
    if training and not update_running:
        return ops.bn_stats(src, 1, None)
    return bn_stats_for(B, name, src, 1, training)


def _double_conv(P, B, names, X, mid, out, training, dsts, save=None, operands=True, update_running=True):
    """DoubleConv over X (zero border 1): returns nothing; dsts = (dst0, dst1) of the second ReLU.  save (dict):
    receives what _double_conv_bwd reads -- without operands, only what the gates and the input gradients read (the
    conv outputs and their statistics), not the conv inputs the weight gradients read"""
    c1, b1, c2, b2 = names
    N, h, w = X.n, X.h, X.w
    dev = X.t.device
    t = Buf.empty(N, h, w, mid, 0, dev)
    conv_fwd(P, c1, X, 1, 3, 1, t)
    mean, invstd = _stats(B, b1, t, training, update_running)
    a = Buf.zeros(N, h, w, mid, 1, dev)
    ops.bn_apply(t, 1, mean, invstd, P[b1 + ".weight"], P[b1 + ".bias"], None, FG_ACT_RELU, a)
    u = Buf.empty(N, h, w, out, 0, dev)
    conv_fwd(P, c2, a, 1, 3, 1, u)
    mean2, invstd2 = _stats(B, b2, u, training, update_running)
    ops.bn_apply(u, 1, mean2, invstd2, P[b2 + ".weight"], P[b2 + ".bias"], None, FG_ACT_RELU, dsts[0],
                 FG_ACT_RELU if dsts[1] is not None else 0, dsts[1])
    if save is not None:
        save.update(t=t, m1=mean, i1=invstd, u=u, m2=mean2, i2=invstd2)
        if operands:
            save.update(x=X, a=a)


def _convT2(P, name, X, Y):
    """ConvTranspose2d(k=2, s=2) over X (border >= 1) into Y (Buf or Slice): four single-tap phases"""
    convT_fwd(P, name, X, Y, 2, 0)


def unet_logits(P, B, X0, training=True, save=False, update_running=True):
    """Forward of UNet(3, 1) over X0 (Buf: the [0, 1] image in channels 0..2 of 4, zero border 1).
    Returns the logits Buf [N, H, W, 4] (channel 0); with save=True, (logits, S): S holds the activations
    unet_backward reads (nothing is kept otherwise).  save="input": the state of unet_backward(param_grads=False)
    only -- the pre-BatchNorm conv outputs with their statistics and the max-pool sources, not the conv and
    ConvTranspose inputs that only weight gradients read.  update_running=False (with training): batch statistics
    that leave running_mean, running_var and num_batches_tracked untouched (a frozen network evaluated as the
    reference evaluates it)."""
    N, H, W = X0.n, X0.h, X0.w
    check_input_size(H, W)
    dev = X0.t.device
    enc, dec, head = layer_names()
    full = save != "input"                                           # (with save) the weight gradients' operands too
    S = dict(N=N, H=H, W=W, training=training, operands=full, enc=[{} for _ in range(5)],
             dec=[{} for _ in range(4)]) if save else None
    cats = [Buf.zeros(N, H >> k, W >> k, 2 * ENC[k], 1, dev) for k in range(4)]     # decoder inputs by level
    X = X0
    for k in range(5):
        h, w = H >> k, W >> k
        if k < 4:
            x = Buf.empty(N, h, w, ENC[k], 0, dev)                 # max-pool source
            _double_conv(P, B, enc[k], X, ENC[k], ENC[k], training, (x, Slice(cats[k], 0, ENC[k])),
                         S["enc"][k] if save else None, full, update_running)
            X = Buf.zeros(N, h // 2, w // 2, ENC[k], 1, dev)
            ops.maxpool2(x, X)
        else:
            x = Buf.zeros(N, h, w, ENC[k], 1, dev)
            _double_conv(P, B, enc[k], X, ENC[k], ENC[k], training, (x, None), S["enc"][k] if save else None, full,
                         update_running)
            X = x
        if save and (full or k < 4):
            S["enc"][k]["out"] = x                                 # the level output (k < 4: the max-pool source)
    for i, (up, names) in enumerate(dec):                            # up1 .. up4
        k = 3 - i                                                    # the encoder level it joins
        c = ENC[k]
        _convT2(P, up, X, Slice(cats[k], c, c))
        last = i == len(dec) - 1
        y = Buf.zeros(N, H >> k, W >> k, c, 0 if last else 1, dev)
        _double_conv(P, B, names, cats[k], c, c, training, (y, None), S["dec"][i] if save else None, full,
                     update_running)
        if save and full:
            S["dec"][i].update(xin=X, out=y)                       # the ConvTranspose input, the level output
        X = y
    logits = Buf.empty(N, H, W, 4, 0, dev)
    conv_fwd(P, head, X, 0, 1, 1, logits)
    return (logits, S) if save else logits


def _bn_bwd(G, P, name, gA, gB, src, mean, invstd, dst, fixed, param_grads):
    """BatchNorm + ReLU backward of one DoubleConv half: through the batch statistics, or (fixed: an eval-mode
    forward) through the fixed ones; without param_grads the gamma / beta sums are not formed"""
    gg, gb = (G.get(name + ".weight"), G.get(name + ".bias")) if param_grads else (None, None)
    actB = FG_ACT_RELU if gB is not None else 0
    if fixed:
        ops.bn_bwd_fixed(gA, FG_ACT_RELU, gB, actB, src, mean, invstd, P[name + ".weight"], P[name + ".bias"], dst,
                         gg, gb, G.acc)
    else:
        ops.bn_bwd(gA, FG_ACT_RELU, gB, actB, src, 1, mean, invstd, P[name + ".weight"], P[name + ".bias"], None, dst,
                   gg, gb, G.acc)


def _double_conv_bwd(P, G, names, D, gA, gB=None, need_input=True, split=None, fixed=False, param_grads=True):
    """Backward of _double_conv from its saved tensors D.  The gradient of the DoubleConv's output is
    gA * relu' (+ gB * relu': an encoder level's two consumers).  Returns the input gradient (None when not
    needed: inc's image), as one Buf or, with split=c, as the two Bufs of its channels [0, c) and [c, 2c) (a decoder
    level's cat: the skip half and the ConvTranspose half), both written by one launch.  fixed: the forward ran on
    fixed (eval-mode) statistics.  param_grads=False: input gradients only (D then needs no conv inputs)."""
    c1, b1, c2, b2 = names
    u, t = D["u"], D["t"]
    N, h, w = u.n, u.h, u.w
    dev = u.t.device
    g_u = Buf.empty(N, h, w, u.c, 1, dev)                  # zero border 1: the full correlation of a 3x3, pad 1
    _bn_bwd(G, P, b2, gA, gB, u, D["m2"], D["i2"], g_u, fixed, param_grads)
    ops.zero_border(g_u)
    if param_grads:
        wgrad_conv(P, G, c2, g_u, D["a"], 1, 3, 1)
    g_a = Buf.empty(N, h, w, t.c, 0, dev)
    dgrad_s1(P, c2, g_u, 1, 3, g_a)
    g_t = Buf.empty(N, h, w, t.c, 1, dev)
    _bn_bwd(G, P, b1, g_a, None, t, D["m1"], D["i1"], g_t, fixed, param_grads)
    ops.zero_border(g_t)
    if param_grads:
        wgrad_conv(P, G, c1, g_t, D["x"], 1, 3, 1)
    if not need_input:
        return None
    wt = P[c1 + ".weight"]
    c_in = wt.shape[1]
    if split is None:
        # (inc: 3 image channels in a 4-channel buffer, the engine writing 3 -- as the head writes 1 of 4)
        g_x = Buf.empty(N, h, w, c_in, 0, dev) if c_in % 4 == 0 else Buf.zeros(N, h, w, PL.rup(c_in, 4), 0, dev)
        dgrad_s1(P, c1, g_t, 1, 3, g_x)
        return g_x
    assert c_in == 2 * split
    halves, probs = [], []
    for c0 in (0, split):
        g_h = Buf.empty(N, h, w, split, 0, dev)
        m = PL.wmap_conv_dgrad_s1_part(wt.shape, g_t.c, c0, split)
        probs.append(PL.conv_problem(g_t, 1, 3, 1, ops.pack_weight(wt, m), m, g_h))
        halves.append(g_h)
    ops.conv(probs)
    return halves


def _convT2_bwd(P, G, name, xin, g_y, param_grads=True):
    """Backward of a decoder level's ConvTranspose2d(k=2, s=2, p=0), weight (I, O, 2, 2): g_y [N, 2h, 2w, O] (no
    border needed: the four taps tile the output) -> the gradient of xin [N, h, w, I]; weight and bias gradients
    into G (param_grads=False: neither, and xin is not read)"""
    wt = P[name + ".weight"]
    g_x = Buf.empty(g_y.n, g_y.h // 2, g_y.w // 2, wt.shape[0], 0, g_y.t.device)
    convT_bwd(P, G, name, xin, g_y, 2, 0, g_x, param_grads=param_grads, bias_channels=wt.shape[1])   # K = 4 O
    return g_x


EVAL_BACKWARD = ("floodgan: the segmentation UNet's backward runs through the batch statistics of training-mode "
                 "BatchNorm (models/segmentation_model.py:259 trains under model.train()); a backward in .eval() mode "
                 "is not implemented")


def unet_backward(P, S, g_logits, grads_into=None, choices=None, *, input_grad=False, param_grads=True):
    """Explicit backward of unet_logits(save=True).  g_logits: Buf [N, H, W, >= 4], dL/d(logits) in channel 0.
    Returns {parameter name: gradient} (written into grads_into[name] when given).  A forward in training mode goes
    back through its batch statistics, one in eval mode (S["training"] False) through the fixed statistics it used
    (fg_bn_bwd_fixed).  input_grad=True: also the gradient of the input image -- inc's first conv's input gradient on
    the conv engine, a Buf [N, H, W, 4] (channels 0..2) under the key "input".  param_grads=False: no weight, bias or
    BatchNorm parameter gradient is formed (a frozen network inside a loss); S may then come from
    unet_logits(save="input").  choices (dict, test instrumentation): receives {"pool<k>": uint8 NCHW} -- the window
    position each max-pool gradient went to."""
    if param_grads and not S["operands"]:
        raise RuntimeError("unet_backward: parameter gradients need the conv inputs, which a forward saved with "
                           "save=\"input\" does not keep (use save=True, or param_grads=False)")
    fixed = not S["training"]
    N, H, W = S["N"], S["H"], S["W"]
    if (g_logits.n, g_logits.h, g_logits.w) != (N, H, W):
        raise RuntimeError(f"unet_backward: logits gradient {g_logits.n}x{g_logits.h}x{g_logits.w} for a saved "
                           f"forward of {N}x{H}x{W}")
    dev = g_logits.t.device
    G = Grads(P, grads_into)
    enc, dec, head = layer_names()
    # ---- OutConv 1x1, 64 -> 1 (weight + bias, then the input gradient)
    if param_grads:
        y = S["dec"][3]["out"]
        ops.conv1x1_wgrad(g_logits, y, 1, G.get(head + ".weight"), G.get(head + ".bias"), G.acc)
    g = Buf.empty(N, H, W, 64, 0, dev)
    ops.conv1x1_dgrad(g_logits, P[head + ".weight"], 1, g)
    # ---- decoder, up4 .. up1
    g_skip = {}
    for i in reversed(range(4)):
        k = 3 - i
        up, names = dec[i]
        D = S["dec"][i]
        g_skip[k], g_up = _double_conv_bwd(P, G, names, D, g, split=ENC[k], fixed=fixed, param_grads=param_grads)
        g = _convT2_bwd(P, G, up, D.get("xin"), g_up, param_grads)
    # ---- encoder, down4 .. inc
    for k in range(4, -1, -1):
        E = S["enc"][k]
        if k == 4:
            gA, gB = g, None
        else:
            src = E["out"]
            gA = Buf.empty(N, src.h, src.w, src.c, 0, dev)
            ch = None
            if choices is not None:
                ch = torch.empty(N, src.h // 2, src.w // 2, src.c, dtype=torch.uint8, device=dev)
                choices[f"pool{k}"] = ch.permute(0, 3, 1, 2)
            ops.maxpool2_bwd(src, g, gA, ch)
            gB = g_skip.pop(k)
        g = _double_conv_bwd(P, G, enc[k], E, gA, gB, need_input=k > 0 or input_grad, fixed=fixed,
                             param_grads=param_grads)
    if input_grad:
        G.out["input"] = g
    return G.out


def unet_decisions(S):
    """The forward's ReLU decisions in a saved forward, keyed "<BatchNorm name>" -> NCHW bool on the host (test
    instrumentation: tests/seg_train_oracle.py teacher-forces them; the max-pool choices come from
    unet_backward(choices=...), which makes them)"""
    enc, dec, _ = layer_names()
    out = {}
    for names, D in list(zip(enc, S["enc"])) + [(n, D) for (_, n), D in zip(dec, S["dec"])]:
        out[names[1]] = decided(D["a"])
        out[names[3]] = decided(D["out"])
    return out


def _nchw(buf, c):
    """channels 0 .. c of a Buf's interior as an [N, c, H, W] view"""
    return buf.interior()[..., :c].permute(0, 3, 1, 2)


def unit_image(x, buf=None, nchw=True):
    """torch.clamp((x + 1) * 0.5, 0, 1) of an [N, C, H, W] generator output / target: (NCHW tensor or
    None, U-Net input Buf or None)"""
    require_device(x, "image")
    N, C, H, W = x.shape
    out = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device) if nchw else None
    if buf is True:
        buf = Buf.zeros(N, H, W, PL.rup(C, 4), 1, x.device)
    from . import _lib as L
    L.check(L.load().fg_unit_image(ops.sview(x), N, C, H, W, L.ptr(out), ops.view(buf), L.stream_handle()),
            "unit_image")
    ops.wrote(buf)
    return out, buf


# ------------------------------------------------------------------------------------------ modules

def _sd_keys(module):
    return [k for k, _ in module.named_parameters()]


class _UNetFn(torch.autograd.Function):
    """forward: the native executor; activations are saved only when a gradient can be computed from them: the
    caller's grad mode on (autograd runs forward with grad mode off, so it arrives as `save`), a parameter needing
    one, and the module in train() mode.  backward: unet_backward on the parameters autograd saved (an in-place
    update of one between forward and backward is caught by its version check).  With module.input_grad set, the
    input image may need a gradient too (alone: the save="input" state), and eval() mode saves as train() does"""

    @staticmethod
    def forward(ctx, module, save, x, *params):
        keys = _sd_keys(module)
        P = dict(zip(keys, params))
        B = dict(module.named_buffers())
        _, X0 = unit_image_passthrough(x)
        wants_x, wants_p = bool(save and ctx.needs_input_grad[2]), bool(save and any(ctx.needs_input_grad[3:]))
        full = module.input_grad                         # the switch: input gradient, and a backward in eval mode
        if wants_x and not full:
            raise RuntimeError("floodgan: the segmentation UNet does not compute the gradient of its input image "
                               "(pass an input with requires_grad=False, or set UNet.input_grad = True)")
        ctx.S, ctx.eval_mode = None, wants_p and not module.training and not full
        if (wants_p and module.training) or (full and (wants_x or wants_p)):
            logits, ctx.S = unet_logits(P, B, X0, module.training, save=True if wants_p else "input")
            ctx.keys, ctx.wants = keys, (wants_x, wants_p)
            ctx.save_for_backward(*params)
        else:
            logits = unet_logits(P, B, X0, module.training)
        return _nchw(logits, 1).contiguous()

    @staticmethod
    def backward(ctx, g):
        if ctx.eval_mode:
            raise RuntimeError(EVAL_BACKWARD)
        if ctx.S is None:
            raise RuntimeError("floodgan: segmentation UNet backward without a saved forward")
        P, S = dict(zip(ctx.keys, ctx.saved_tensors)), ctx.S
        ctx.S = None                                     # (a second backward through the same graph is an error)
        wants_x, wants_p = ctx.wants
        g_logits = Buf.empty(S["N"], S["H"], S["W"], 4, 0, g.device)
        ops.pack_input(g, 1, None, 0, g_logits, 0, S["N"], FG_PAD_ZERO)
        grads = unet_backward(P, S, g_logits, input_grad=wants_x, param_grads=wants_p)
        g_x = _nchw(grads["input"], 3).contiguous() if wants_x else None
        return (None, None, g_x) + tuple(grads[k] if need and wants_p else None
                                         for k, need in zip(P, ctx.needs_input_grad[3:]))


def unit_image_passthrough(x):
    """pack an [N, 3, H, W] image as the U-Net's NHWC input (no value change)"""
    require_device(x, "segmentation input")
    N, C, H, W = x.shape
    if C != 3:
        raise RuntimeError(f"segmentation UNet takes 3-channel images (got {C})")
    buf = Buf.zeros(N, H, W, 4, 1, x.device)
    ops.pack_input(x, 3, None, 0, buf, 0, N, FG_PAD_ZERO)
    return None, buf


class DoubleConv(nn.Module):
    """models/model_architectures.py:540-553"""

    def __init__(self, in_channels, out_channels, mid_channels=None):
        super().__init__()
        if not mid_channels:
            mid_channels = out_channels
        self.double_conv = nn.Sequential(
            nn.Conv2d(in_channels, mid_channels, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(mid_channels),
            nn.ReLU(inplace=True),
            nn.Conv2d(mid_channels, out_channels, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(out_channels),
            nn.ReLU(inplace=True))

    def forward(self, x):
        raise RuntimeError("floodgan: DoubleConv runs inside its UNet's native forward")


class Down(nn.Module):
    """models/model_architectures.py:555-562"""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.maxpool_conv = nn.Sequential(nn.MaxPool2d(2), DoubleConv(in_channels, out_channels))

    def forward(self, x):
        raise RuntimeError("floodgan: Down runs inside its UNet's native forward")


class Up(nn.Module):
    """models/model_architectures.py:564-580 (bilinear=False: ConvTranspose2d(in, in // 2, 2, 2))"""

    def __init__(self, in_channels, out_channels, bilinear=True):
        super().__init__()
        if bilinear:
            self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
            self.conv = DoubleConv(in_channels, out_channels, in_channels // 2)
        else:
            self.up = nn.ConvTranspose2d(in_channels, in_channels // 2, kernel_size=2, stride=2)
            self.conv = DoubleConv(in_channels, out_channels)

    def forward(self, x1, x2):
        raise RuntimeError("floodgan: Up runs inside its UNet's native forward")


class OutConv(nn.Module):
    """models/model_architectures.py:582-587"""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=1)

    def forward(self, x):
        raise RuntimeError("floodgan: OutConv runs inside its UNet's native forward")


class UNet(nn.Module):
    """models/model_architectures.py:508-538 -- same modules, registration order and state_dict keys;
    forward = the native executor (logits [N, 1, H, W]); in train() mode it trains under stock loss.backward() and
    any torch optimizer (no gradient of the input image; no backward in eval() mode).  Setting input_grad = True
    lifts both limits: an input that requires a gradient gets one, and a backward in eval() mode runs through the
    fixed running statistics (parameter gradients included)."""

    input_grad = False

    def __init__(self, n_channels=3, n_classes=1, bilinear=False):
        super().__init__()
        self.n_channels, self.n_classes, self.bilinear = n_channels, n_classes, bilinear
        self.inc = DoubleConv(n_channels, 64)
        self.down1 = Down(64, 128)
        self.down2 = Down(128, 256)
        self.down3 = Down(256, 512)
        factor = 2 if bilinear else 1
        self.down4 = Down(512, 1024 // factor)
        self.up1 = Up(1024, 512 // factor, bilinear)
        self.up2 = Up(512, 256 // factor, bilinear)
        self.up3 = Up(256, 128 // factor, bilinear)
        self.up4 = Up(128, 64, bilinear)
        self.outc = OutConv(64, n_classes)

    def _check(self):
        if self.bilinear or self.n_channels != 3 or self.n_classes != 1:
            raise NotImplementedError("floodgan's segmentation executor covers the reference's UNet(3, 1, "
                                      "bilinear=False) (models/segmentation_model.py:55)")

    def forward(self, x):
        self._check()
        return _UNetFn.apply(self, torch.is_grad_enabled(), x, *[p for _, p in self.named_parameters()])

    def logits_from_buf(self, X0):
        """logits Buf from a prepared input Buf (the evaluation path: unit_image writes it directly)"""
        self._check()
        P = dict(self.named_parameters())
        B = dict(self.named_buffers())
        with torch.no_grad():
            return unet_logits(P, B, X0, self.training)


def initialise_weights(m):
    """models/segmentation_model.py:73-84 (the GAN's initialise_weights)"""
    classname = m.__class__.__name__
    if hasattr(m, "weight") and (classname.find("Conv") != -1 or classname.find("Linear") != -1):
        nn.init.normal_(m.weight.data, 0.0, 0.02)
        if hasattr(m, "bias") and m.bias is not None:
            nn.init.constant_(m.bias.data, 0.0)
    elif classname.find("BatchNorm2d") != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0.0)


class SegStep:
    """One segmentation training iteration (models/segmentation_model.py:261-274) on device tensors x [N, 3, H, W]
    and true_mask [N, 1, H, W]: native forward, BCE-with-logits with the accuracy count (fg_bce_logits), explicit
    backward into the parameters' .grad, optimizer step.  Returns one 16-byte device tensor holding (loss, number
    of correct mask elements): a single copy brings both to the host (SegStep.read)."""

    def __init__(self, model, optimizer):
        self.model, self.opt = model, optimizer
        self.P = dict(model.named_parameters())
        # test instrumentation: when True, each call stores its ReLU decisions, max-pool choices and logits in
        # self.decisions ({"relu": {...}, "pool": {...}, "logits": NCHW host tensor})
        self.record_decisions = False
        self.decisions = None

    def __call__(self, x, true_mask):
        self.model._check()
        require_device(true_mask, "segmentation target")
        N, _, H, W = x.shape
        dev = x.device
        _, X0 = unit_image_passthrough(x)
        logits, S = unet_logits(self.P, dict(self.model.named_buffers()), X0, self.model.training, save=True)
        res = torch.empty(2, dtype=torch.int64, device=dev)         # [0]: the fp32 loss in its low half, [1]: count
        g = Buf.empty(N, H, W, 4, 0, dev)
        ops.bce_logits(logits, true_mask.contiguous(), 1.0 / (N * H * W), g, res[:1].view(torch.float32), res[1:])
        for p in self.P.values():                                   # optimizer.zero_grad(): every gradient is
            if p.grad is None:                                      # overwritten below
                p.grad = torch.empty_like(p)
        choices = {} if self.record_decisions else None
        if self.record_decisions:
            self.decisions = dict(relu=unet_decisions(S), pool=choices,
                                  logits=_nchw(logits, 1).cpu())
        unet_backward(self.P, S, g, grads_into={k: p.grad for k, p in self.P.items()}, choices=choices)
        del S
        if choices:
            self.decisions["pool"] = {k: v.cpu() for k, v in choices.items()}
        self.opt.step()
        return res

    @staticmethod
    def read(res, numel):
        """(loss, accuracy) on the host from a step's result: one device-to-host copy"""
        host = res.cpu()
        return float(host[:1].view(torch.float32)[0]), int(host[1]) / numel


# ------------------------------------------------------------------------------------------ the flood-mask loss

def _flood_mask_pass(P, B, fake, real, batch_stats, save):
    """The forward half of the flood-mask loss on two [N, 3, H, W] images in [-1, 1]: fg_unit_image on both, the
    frozen U-Net on both (the `real` pass keeps nothing; the `fake` pass keeps the save="input" state when `save`),
    fg_flood_mask_bce of the fake logits against the mask of the real ones.  Returns (result, g, S, logits, ref):
    result = the 16-byte (loss, agreeing pixels) tensor SegStep.read unpacks, g = dL/d(logits) for the mean loss."""
    N, _, H, W = fake.shape
    _, F0 = unit_image(fake, buf=True, nchw=False)
    _, R0 = unit_image(real, buf=True, nchw=False)
    ref = unet_logits(P, B, R0, batch_stats, update_running=False)
    out = unet_logits(P, B, F0, batch_stats, save="input" if save else False, update_running=False)
    logits, S = out if save else (out, None)
    res = torch.empty(2, dtype=torch.int64, device=fake.device)
    g = Buf.empty(N, H, W, 4, 0, fake.device)
    ops.flood_mask_bce(logits, ref, 1.0 / (N * H * W), g, res)
    return res, g, S, logits, ref


class _FloodMaskFn(torch.autograd.Function):
    """FloodMaskLoss as one autograd node: differentiable in `fake` only; the U-Net's parameters are constants"""

    @staticmethod
    def forward(ctx, owner, save, fake, real):
        P, B = owner._state()
        wants = bool(save and ctx.needs_input_grad[2])
        res, g, S, _, _ = _flood_mask_pass(P, B, fake, real, owner.batch_stats, wants)
        owner._last = (res, g.n * g.h * g.w)
        ctx.state = (P, S, g) if wants else None
        if wants:
            ctx.save_for_backward(fake)
        return res[:1].view(torch.float32)[0].clone()

    @staticmethod
    def backward(ctx, g_loss):
        if ctx.state is None:
            raise RuntimeError("floodgan: FloodMaskLoss backward without a saved forward")
        (fake,) = ctx.saved_tensors
        (P, S, g), ctx.state = ctx.state, None           # (a second backward through the same graph is an error)
        g_in = unet_backward(P, S, g, input_grad=True, param_grads=False)["input"]
        g_fake = torch.empty_like(fake)
        ops.unit_image_bwd(g_in, fake, g_fake)
        return None, None, g_fake.mul_(g_loss), None


class _FusedFloodMaskTerm:
    """FloodMaskLoss as PairedStep.fake_loss: called as term(fake, real, g_fake, scale) between the L1 term and the
    G step's discriminator backward, it adds scale * dL/d(fake) into g_fake and returns weight * L as a device
    tensor of one element (no host synchronisation)"""

    def __init__(self, loss, weight):
        self.loss, self.weight = loss, float(weight)

    def __call__(self, fake, real, g_fake, scale):
        loss = self.loss
        loss._check_images(fake, real)
        P, B = loss._state()
        res, g, S, _, _ = _flood_mask_pass(P, B, fake, real, loss.batch_stats, True)
        loss._last = (res, g.n * g.h * g.w)
        g_in = unet_backward(P, S, g, input_grad=True, param_grads=False)["input"]
        ops.unit_image_bwd(g_in, fake, g_fake, scale=scale, accumulate=True)
        return res[:1].view(torch.float32)[:1] * self.weight


class FloodMaskLoss(nn.Module):
    """The score the evaluation gives a generator, as a loss: binary cross-entropy of the segmentation U-Net's flood
    logits of `fake` against the flood mask the same U-Net sees in `real` (floodgan.evaluate: MaskConfusion counts
    the agreement of exactly these two masks).  seg_model: a drop-in UNet, a SegmentationModel or a checkpoint path;
    its parameters and buffers are never written.  batch_stats=False: BatchNorm on the running statistics (eval
    mode); True: on the statistics of each batch, as the reference evaluates the model -- the running statistics
    and num_batches_tracked stay untouched in both.  forward(fake, real): two [N, 3, H, W] device images in
    [-1, 1] -> a scalar, differentiable with respect to `fake` only; nothing is saved when `fake` needs no
    gradient or under torch.no_grad()."""

    def __init__(self, seg_model, batch_stats=False):
        super().__init__()
        import os
        if isinstance(seg_model, (str, os.PathLike)):
            from .evaluate import segmentation_model
            seg_model = segmentation_model(os.fspath(seg_model))
        elif isinstance(seg_model, SegmentationModel):
            seg_model = seg_model.model
        if not isinstance(seg_model, UNet):
            raise TypeError("FloodMaskLoss takes a floodgan UNet, a SegmentationModel or a checkpoint path "
                            f"(got {type(seg_model).__name__})")
        seg_model._check()
        self.seg, self.batch_stats = seg_model, bool(batch_stats)
        self._last = None

    def _state(self):
        return dict(self.seg.named_parameters()), dict(self.seg.named_buffers())

    @staticmethod
    def _check_images(fake, real):
        require_device(fake, "flood-mask loss image")
        require_device(real, "flood-mask loss target")
        if fake.dim() != 4 or fake.shape[1] != 3 or fake.shape != real.shape:
            raise RuntimeError(f"FloodMaskLoss takes two [N, 3, H, W] images (got {tuple(fake.shape)} and "
                               f"{tuple(real.shape)})")

    def forward(self, fake, real):
        self._check_images(fake, real)
        return _FloodMaskFn.apply(self, torch.is_grad_enabled(), fake, real.detach())

    def read(self):
        """(loss, fraction of agreeing mask pixels) of the last call: one device-to-host copy"""
        if self._last is None:
            raise RuntimeError("FloodMaskLoss.read before any call")
        return SegStep.read(*self._last)

    @property
    def agreement(self):
        """the last call's fraction of pixels whose two flood masks agree (MaskConfusion's Accuracy of the batch)"""
        return self.read()[1]

    def logits(self, fake, real):
        """the two logits tensors [N, 1, H, W] the loss is formed from (nothing is saved)"""
        self._check_images(fake, real)
        with torch.no_grad():
            P, B = self._state()
            _, _, _, z, r = _flood_mask_pass(P, B, fake, real, self.batch_stats, False)
        return tuple(_nchw(b, 1).contiguous() for b in (z, r))

    def fused_term(self, weight):
        """this loss as the fake_loss hook of the fused paired step (PairedStep / Pix2PixStep)"""
        return _FusedFloodMaskTerm(self, weight)


class SegmentationModel:
    """models/segmentation_model.py:19-177, 244-277: the UNet, initialised as the reference does (no reseeding: it
    draws from the global generator), optionally loaded from a checkpoint ({"model": state_dict, "current_epoch",
    "num_epochs", "all_losses", "all_accuracies"}, read with weights_only=True; the reference's checkpoints load
    here and these load there).  train=True: BCE-with-logits (fg_bce_logits), FusedAdam(1e-4, (0.5, 0.999)), the
    LambdaLR of lambda_rule, starting_epoch resumed from the checkpoint; train_model() runs the fused SegStep.
    The loaders come from floodgan.data.create_masks_dataset when data_path is given, or are assigned
    (train_loader / val_loader / test_loader: iterables of (image, mask, names)).  Every keyword of the reference's
    constructor is accepted (segment.py passes them all); staged_loader=True (not a keyword of the reference's) asks
    create_masks_dataset for MaskTileLoaders, whose batches are the same and arrive on the device.  Pictures go
    through floodgan.render: save_images_interval
    writes the sample sheet (plot_sample_images(num_images=10)) every that many epochs, plot_mask_image(path) the
    predicted mask of one image; the constructor's plot_mask_image= is kept in mask_image_path for the caller
    (segment.py calls the method itself); both need a data_path to write under and raise without one.  The
    loss-curve figure (plot_loss) is a matplotlib line chart and is not drawn here."""

    def __init__(self, data_path=None, pretrained_model_path=None, train=False, device="cuda", seed=47,
                 dataset_subset="usa", num_epochs=100, train_on_all=False, save_model_interval=0, verbose=True,
                 save_images_interval=0, plot_mask_image=None, use_test_data=False,
                 csv_path="metadata/masks_metadata.csv", staged_loader=False):
        if (save_images_interval != 0 or plot_mask_image) and data_path is None:
            # the pictures are written under {data_path}/images (models/segmentation_model.py:102, :205)
            raise NotImplementedError("floodgan: the segmentation model's pictures (save_images_interval != 0: "
                                      "plot_sample_images; plot_mask_image) are written under data_path; without "
                                      "one they are out of scope: pass data_path, or save_images_interval=0 and "
                                      "plot_mask_image=None")
        self.save_images_interval, self.use_test_data = save_images_interval, use_test_data
        self.mask_image_path = plot_mask_image
        self.data_path, self.pretrained_model_path, self.seed = data_path, pretrained_model_path, seed
        self.dataset_subset, self.train_on_all, self.train = dataset_subset, train_on_all, train
        self.save_model_interval, self.verbose, self.csv_path = save_model_interval, verbose, csv_path
        self.device, self.staged_loader = device, staged_loader
        self.starting_epoch = 1
        self.current_epoch, self.num_epochs, self.all_losses, self.all_accuracies = 1, num_epochs, [], []
        self.model = UNet().apply(initialise_weights).to(device)
        if pretrained_model_path:
            saved = torch.load(pretrained_model_path, map_location="cpu", weights_only=True)
            self.current_epoch, self.num_epochs = saved["current_epoch"], saved["num_epochs"]
            self.model.load_state_dict(saved["model"])
            self.all_losses, self.all_accuracies = saved["all_losses"], saved["all_accuracies"]
        self.train_loader = self.val_loader = self.test_loader = None
        self._step = None
        if train:
            from torch.optim import lr_scheduler

            from .optim import FusedAdam
            self.starting_epoch = self.current_epoch
            self.optimizer = FusedAdam(self.model.parameters(), lr=0.0001, betas=(0.5, 0.999))
            self.scheduler = lr_scheduler.LambdaLR(self.optimizer, lr_lambda=self.lambda_rule)
            if data_path is not None:
                self.train_loader, self.val_loader, self.test_loader = self._loaders()

    def _loaders(self):
        from .data import create_masks_dataset
        return create_masks_dataset(self.dataset_subset, self.data_path, self.train_on_all, csv_path=self.csv_path,
                                    staged=self.staged_loader, device=self.device)

    def _eval_loader(self, use_test_data):
        """the validation (or test) loader: the assigned one, else built from data_path"""
        val_loader, test_loader = self.val_loader, self.test_loader
        if val_loader is None and test_loader is None and self.data_path is not None:
            _, val_loader, test_loader = self._loaders()
        loader = test_loader if use_test_data else val_loader
        if loader is None:
            raise RuntimeError("no evaluation data: pass data_path or assign val_loader / test_loader")
        return loader

    def lambda_rule(self, epoch):
        """models/segmentation_model.py:86-92: constant for the first half of the epochs, then linear decay"""
        return 1.0 - max(0, epoch + 1 - (self.num_epochs / 2)) / float((self.num_epochs / 2) + 1)

    def create_path(self, save_type):
        """models/segmentation_model.py:94-105"""
        from datetime import datetime
        ext = {"image": ".png", "figure": ".png", "model": ".pth.tar", "metric": ".csv"}[save_type]
        now = str(datetime.now())[:-7].replace(" ", "-").replace(":", "-")
        return (f"{self.data_path}/{save_type}s/"
                f"SegmentationModel_epoch{self.current_epoch if self.train else self.current_epoch - 1}_"
                f"{self.dataset_subset}Data_date{now}{ext}")

    @property
    def step_fn(self):
        if self._step is None:
            self._step = SegStep(self.model, self.optimizer)
        return self._step

    def train_model(self):
        """models/segmentation_model.py:250-277 on the fused device step; loss and accuracy reach the host once
        per batch"""
        if not self.train:
            raise RuntimeError("SegmentationModel.train_model needs train=True")
        if self.train_loader is None:
            raise RuntimeError("no training data: pass data_path (floodgan.data.create_masks_dataset, as "
                               "models/segmentation_model.py:69-71) or assign train_loader (an iterable of "
                               "(image, mask, names))")
        for epoch in range(self.starting_epoch, self.num_epochs + 1):
            t0 = time.time()
            losses, accuracies = [], []
            self.model.train()
            for input_image, true_mask, _ in self.train_loader:
                input_image = input_image.to(self.device, non_blocking=True)
                true_mask = true_mask.to(self.device, non_blocking=True)
                loss, acc = SegStep.read(self.step_fn(input_image, true_mask), true_mask.numel())
                losses.append(loss)
                accuracies.append(acc)
            self.scheduler.step()
            self.save_results(epoch, losses, accuracies, t0)

    def checkpoint(self, epoch):
        """the reference's checkpoint dict (models/segmentation_model.py:122-127)"""
        return {"current_epoch": epoch + 1, "num_epochs": self.num_epochs, "model": self.model.state_dict(),
                "all_losses": self.all_losses, "all_accuracies": self.all_accuracies}

    def save_results(self, epoch, losses, accuracies, epoch_start_time):
        """models/segmentation_model.py:107-134: per-epoch means, checkpoint and, every save_images_interval epochs,
        the sample sheet (plot_sample_images(num_images=10)); the loss-curve figure (plot_loss) is not drawn"""
        import os
        self.current_epoch = epoch
        self.all_losses.append(float(np.mean(losses)))
        self.all_accuracies.append(float(np.mean(accuracies)))
        if self.verbose:
            print(f"Epoch {epoch} ({time.time() - epoch_start_time:.2f} seconds) | Loss = {self.all_losses[-1]:.2f} | "
                  f"Accuracy = {self.all_accuracies[-1]:.2f}")
        path = None
        if self.save_model_interval != 0 and epoch % self.save_model_interval == 0:
            path = self.create_path("model")
            if self.verbose:
                print(f"Saving flood segmentation model to {path}")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            torch.save(self.checkpoint(epoch), path)
        if self.save_images_interval != 0 and epoch % self.save_images_interval == 0:
            self.plot_sample_images(num_images=10, use_test_data=False)
        return path

    def calculate_metrics(self, use_test_data=False):
        """models/segmentation_model.py:136-177: the binary mask metrics of the model's flood masks against the
        true masks (t > 0.5) over the validation / test loader, accumulated on the device (MaskConfusion: a true
        mask t > 0.5 is the logit t - 0.5).  Returns the one-row DataFrame the reference prints (and writes it
        under data_path/metrics/ when data_path is set)."""
        import os

        import pandas as pd

        from .evaluate import MaskConfusion
        loader = self._eval_loader(use_test_data)
        conf = MaskConfusion(self.device)
        for input_image, true_mask, _ in loader:
            x = input_image.to(self.device)
            t = true_mask.to(self.device)
            N, _, H, W = x.shape
            pred = self.model.logits_from_buf(unit_image_passthrough(x)[1])
            true = Buf.zeros(N, H, W, 4, 0, x.device)
            true.interior()[..., 0] = t[:, 0] - 0.5
            conf.update(pred, true)
        df = pd.DataFrame([(k, v) for k, v in conf.compute().items()]).set_index(0).transpose()
        if self.verbose:
            print(df)
        if self.data_path:
            path = self.create_path("metric")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            df.to_csv(path)
        return df

    # ---- pictures (models/segmentation_model.py:196-242) on floodgan.render

    def plot_mask_image(self, path_to_image):
        """models/segmentation_model.py:196-207: the predicted flood mask of one picture -- a PNG (bytes / 255, its
        first three channels, as plt.imread) or a tile read_tile accepts -- as a "gray" image at
        {data_path}/images/SegmentationMask_{name}_{time}.png.  The mask is decided on the device by the function
        that decides fg_mask_confusion's.  Returns the path."""
        import os
        from datetime import datetime

        from .png import read_image
        from .render import save_image
        image_name = path_to_image.split("/")[-1][:-4]
        if path_to_image.lower().endswith(".png"):
            a = read_image(path_to_image)
            if a.shape[2] < 3:
                raise ValueError(f"plot_mask_image: {path_to_image} has {a.shape[2]} channel(s); an RGB picture is needed")
            a = a[:, :, :3].astype(np.float32) / np.float32(255)
        else:
            from .data import read_tile
            a = read_tile(path_to_image)[:, :, :3]
        x = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))[None].to(self.device)
        logits = self.model.logits_from_buf(unit_image_passthrough(x)[1])
        now = str(datetime.now())[:-7].replace(" ", "-").replace(":", "-")
        path = f"{self.data_path}/images/SegmentationMask_{image_name}_{now}.png"
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if self.verbose:
            print(f"Saving segmentation mask for '{image_name}' to {path}")
        return save_image(path, logits, "mask_logits")

    def plot_sample_images(self, num_images, use_test_data=False):
        """models/segmentation_model.py:209-242: one sheet of the first num_images validation (or test) items, batch
        element 0 of each: input (clip(x, 0, 1)) | true mask (t > 0.5) | predicted mask (sigmoid(logit) > 0.5), at
        create_path("image"), under torch.manual_seed(self.seed).  Returns the path."""
        import os

        from .render import save_sheet
        loader = self._eval_loader(use_test_data)
        xs, ts, ps, names = [], [], [], []
        torch.manual_seed(self.seed)
        for i, (input_image, true_mask, image_name) in enumerate(loader):
            x = input_image.to(self.device)
            t = true_mask.to(self.device)
            logits = self.model.logits_from_buf(unit_image_passthrough(x)[1])
            xs.append(x[:1])
            ts.append(t[:1])
            ps.append(logits.interior()[:1, :, :, 0])
            names.append(image_name[0])
            if i >= num_images - 1:
                break
        if not names:
            raise RuntimeError("plot_sample_images: the loader is empty")
        path = self.create_path("image")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if self.verbose:
            print("Saving sample images to", path)
        self.last_panels = save_sheet(path, [("Input", "rgb_unit", xs), ("Ground Truth Mask", "mask_true", ts),
                                             ("Predicted Mask", "mask_logits", ps)], names)
        return path

    @staticmethod
    def tensor_to_mask(tensor, predicted=True):
        """models/segmentation_model.py:244-248"""
        return (torch.sigmoid(tensor) > 0.5).float() if predicted else (tensor > 0.5).float()
