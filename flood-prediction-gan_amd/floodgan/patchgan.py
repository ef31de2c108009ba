"""The 70x70 PatchGAN discriminator's native forward / backward, shared by its InstanceNorm form
(PairedAttention, the cycle models: floodgan.executor) and its BatchNorm form (Pix2Pix: floodgan.pix2pix).

Reference: models/model_architectures.py:424-441 and :64-85: model.0 conv + LeakyReLU; three conv -> norm ->
LeakyReLU levels (LEVELS); model.11, the one-channel head.  All convs are 4x4, padding 1.

The normalisation is an object `norm` with
  norm.conv_stats                          the level convs' epilogues emit InstanceNorm statistics
  norm.forward(P, conv, e, stats, fp32)    norm + LeakyReLU of the conv output e (stats: the epilogue's, or None)
                                           -> the level's saved state {e, mean, rstd | invstd, a}; a: the
                                           activation, zero border 1; fp32: its reader takes no pre-split operand
  norm.backward(P, G, conv, L, g_a, g_e)   g_a = dL/da -> g_e = dL/de with a zero border, and the norm's (or the
                                           conv bias's) parameter gradients into G (None: none)
It is kept in the saved state, so the backward runs through the norm its forward ran.
"""
import torch

from . import ops
from . import plans as PL
from ._lib import FG_ACT_LRELU, FG_PAD_ZERO
from .layers import Grads, conv_fwd, decided, dgrad_s1, dgrad_s2, wgrad_conv
from .plans import Buf

LEVELS = (("model.2", 2, 128), ("model.5", 2, 256), ("model.8", 1, 512))     # (conv, stride, output channels)


def forward(P, inp, norm, save=True, who="PatchGAN discriminator", tags=None):
    """inp: Buf from executor.disc_pack (zero border 1).  Returns (pred [N,1,ho,wo], saved).  tags: {conv: timer
    tag} of level convs"""
    N, H, W = inp.n, inp.h, inp.w
    dev = inp.t.device
    if H < 24 or W < 24:
        raise RuntimeError(f"{who} needs H, W >= 24 (got {H}x{W})")
    e0 = Buf.empty(N, PL.out_size(H, 4, 2, 1), PL.out_size(W, 4, 2, 1), 64, 1, dev)
    conv_fwd(P, "model.0", inp, 1, 4, 2, e0, act=FG_ACT_LRELU)         # conv + bias + LeakyReLU fused, zero border
    ops.zero_border(e0)
    S = dict(inp=inp, e0=e0, norm=norm)
    prev = e0
    for conv, stride, c in LEVELS:
        e = Buf.empty(N, PL.out_size(prev.h, 4, stride, 1), PL.out_size(prev.w, 4, stride, 1), c, 0, dev)
        st = conv_fwd(P, conv, prev, 1, 4, stride, e, tag=(tags or {}).get(conv), in_stats=norm.conv_stats)
        S[conv] = dict(norm.forward(P, conv, e, st, fp32=conv == LEVELS[-1][0]), x=prev)
        prev = S[conv]["a"]
    pred = torch.empty(N, 1, PL.out_size(prev.h, 4, 1, 1), PL.out_size(prev.w, 4, 1, 1), dtype=torch.float32,
                       device=dev)
    ops.conv_n1_fwd(prev, P["model.11.weight"], P["model.11.bias"], pred)      # GEMV-shaped: fp32 FMA kernel
    return pred, (S if save else None)


def backward(P, S, g_pred, param_grads=True, grads_into=None, input_grad=None, input_grad_channels=None,
             input_grad_accumulate=False, ready=None, raise_e0_slot=False, d0_fast=False):
    """Explicit backward of forward.
    param_grads: compute weight / bias gradients (False in the generator step, where D is
    frozen: models/model.py:636-637).  input_grad: contiguous NCHW tensor whose channels 0 .. count
    receive dL/d(input channels input_grad_channels=(start, count)), written or accumulated.  ready(layer name), when
    given, is called as each layer's gradients are complete (parallel.FlatGrads buckets).
    raise_e0_slot: model.0's LeakyReLU backward also raises its gradient's operand-scale slot (the gradient's border
    holds zeros).  d0_fast: the restricted input gradient on its fp32 kernel (fg_d0_input_grad) where it applies,
    instead of the restricted 4-phase transposed conv on the engine."""
    ready = (ready if param_grads and ready is not None else (lambda name: None))
    inp, norm, e0 = S["inp"], S["norm"], S["e0"]
    N = inp.n
    dev = inp.t.device
    G = Grads(P, grads_into)
    a3 = S[LEVELS[-1][0]]["a"]
    g11 = Buf.empty(N, g_pred.shape[2], g_pred.shape[3], 1, 3, dev)   # zero border 3: the n1 weight-gradient
    ops.pack_input(g_pred, 1, None, 0, g11, 0, N, FG_PAD_ZERO)        # kernel's reach
    if param_grads:
        w11 = P["model.11.weight"]
        ops.conv_n1_wgrad(a3, g11, PL.wmap_wgrad(w11.shape, True, a3.c, 4), G.get("model.11.weight"))   # fp32
        ops.channel_sum(g11, 1, G.get("model.11.bias"))
        ready("model.11")
    g_a = Buf.empty(N, a3.h, a3.w, a3.c, 0, dev)
    dgrad_s1(P, "model.11", g11, 2, 4, g_a)
    for conv, stride, _ in reversed(LEVELS):
        L = S[conv]
        e, x = L["e"], L["x"]
        # zero border: the full correlation of the 4x4 (2 at stride 1; 1 for the phases of stride 2)
        g_e = Buf.empty(N, e.h, e.w, e.c, 2 if stride == 1 else 1, dev)
        norm.backward(P, G if param_grads else None, conv, L, g_a, g_e)
        if param_grads:
            wgrad_conv(P, G, conv, g_e, x, 1, 4, stride)
            ready(conv)
        g_a = Buf.empty(N, x.h, x.w, x.c, 1 if x is e0 else 0, dev)
        if stride == 1:
            dgrad_s1(P, conv, g_e, 2, 4, g_a)
        else:
            dgrad_s2(P, conv, g_e, 4, Y=g_a)
    g_e0 = g_a
    ops.zero_border(g_e0)
    ops.act_bwd(g_e0, e0, FG_ACT_LRELU, border_zero=raise_e0_slot)    # LeakyReLU of model.1
    if param_grads:
        wgrad_conv(P, G, "model.0", g_e0, inp, 1, 4, 2)
        ops.channel_sum(g_e0, 64, G.get("model.0.bias"))
        ready("model.0")
    if input_grad is not None:
        c0, cn = input_grad_channels
        # input_grad: contiguous [N, Ctot, H, W]; D-input channels c0 .. c0+cn land in its channels 0 .. cn
        assert input_grad.is_contiguous() and input_grad.shape[1] >= cn
        if d0_fast and ops.d0_input_grad_ok(g_e0, c0, cn, inp.h, inp.w):
            ops.d0_input_grad(g_e0, P["model.0.weight"], c0, cn, input_grad, input_grad_accumulate)
        else:
            dgrad_s2(P, "model.0", g_e0, 4, y_nchw=(input_grad.view(-1), input_grad.shape[1], inp.h, inp.w),
                     n_base=c0, n_out=cn, accumulate=int(input_grad_accumulate))
    return G.out


def act_decisions(S, lo=0, hi=None):
    """The discriminator's LeakyReLU decisions for images lo..hi of a saved forward (test instrumentation)"""
    out = {"model.0": decided(S["e0"], lo, hi)}
    for conv, _, _ in LEVELS:
        L = S[conv]
        out[conv] = decided(L["a"], lo, hi, pre=L["e"], mean=L["mean"])
    return out
