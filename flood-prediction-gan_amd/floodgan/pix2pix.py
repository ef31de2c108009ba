"""Native forward / backward executors of the Pix2Pix U-Net-256 generator and its BatchNorm PatchGAN
discriminator; the fused iteration is floodgan.model.Pix2PixStep.  The conv launches come
from the layer kit (floodgan.layers); the discriminator is floodgan.patchgan's PatchGAN with DiscBatchNorm.

Reference: models/model_architectures.py:9-62 (Pix2PixGenerator / Pix2PixBlock), :64-85
(Pix2PixDiscriminator), models/model.py:611-651 (train_paired, shared with PairedAttention).

Layout.  Level k = 1 (outermost) .. 8 (innermost) of the U-Net; at input H x W level k's down conv
(4x4, stride 2, no bias) produces D_k at H/2^k.  Every activation lives in an NHWC Buf whose zero
border is the next conv's padding:
  a_{k+1} = LeakyReLU(D_k)      -- level k+1's down-conv input (the in-place LeakyReLU of
                                   Pix2PixBlock.forward's x, :58-62, so the skip carries it too)
  cat_k   = [ReLU(D_k) | ReLU(U_{k+1})]  -- level k's up-conv input: torch.cat([x, model(x)], 1)
                                   followed by the parent's in-place ReLU, as two channel slices of
                                   one buffer, each written by the BatchNorm pass that produces it
  r_8     = ReLU(D_8)           -- the innermost up-conv input
The up convs (ConvTranspose2d 4x4 s2 p1) run as four sub-pixel phase GEMMs; the outermost one adds
its bias and feeds the tanh head.  BatchNorm (training mode: batch statistics, running statistics
updated in place on the module buffers; eval mode: running statistics) is one statistics pass and
one apply pass that also writes the activated copies.  Dropout(0.5) of levels 5-7 is fused into the
BatchNorm apply / backward passes, its keep decisions either
  "device":  a counter-based hash of (seed, element) evaluated in the apply pass and
             recomputed in the backward -- no mask is drawn, stored or copied; one 62-bit seed per
             generator call comes from torch's CPU generator, so torch.manual_seed fixes the masks; or
  "host" (default since round 5): the 0/1 masks torch's CPU generator gives the reference's CPU path (F.dropout:
             empty_like(x).bernoulli_(0.5), innermost level first: 7, 6, 5), bit for bit -- a seeded run then
             reproduces the reference's CPU run (the parity mode).  Round 5: the masks are no longer drawn on
             the host; the device regenerates torch's MT19937 stream from the generator's state with chunked
             jump-ahead (floodgan.torch_rng, csrc/mt19937.hip) and hands the advanced state back to torch.

The discriminator's D(fake) and D(real) of the D step are separate BatchNorm calls in the
reference (:624-628): one 2N-image pass with groups=2 (statistics per half, the running statistics
updated twice, in order).
"""
import torch

from . import ops
from . import patchgan
from . import plans as PL
from . import torch_rng
from ._lib import FG_ACT_LRELU, FG_ACT_RELU, FG_PAD_ZERO, require_device
from .layers import Grads, bn_stats_for, conv_fwd, convT_bwd, convT_fwd, decided, dgrad_s2, wgrad_conv
from .plans import Buf, Slice

N_LEVELS = 8
DROPOUT_LEVELS = (7, 6, 5)          # draw order (innermost first)
DROP_P = 0.5


def level_channels(c_in):
    """(input_nc, inner_nc, outer_nc) of levels 1..8 (models/model_architectures.py:13-19)"""
    return [(c_in, 64, 3), (64, 128, 64), (128, 256, 128), (256, 512, 256)] + [(512, 512, 512)] * 4


def level_prefix(k):
    """state_dict prefix of level k's nn.Sequential: the outermost block is Pix2PixGenerator.model;
    a submodule sits at index 1 of the outermost Sequential and at index 3 of the middle ones"""
    return "model.model." + "1.model." * (k > 1) + "3.model." * max(0, k - 2)


def level_names(k):
    """{'down', 'downnorm', 'up', 'upnorm'} module names of level k (absent where the reference has none)"""
    p = level_prefix(k)
    if k == 1:
        return dict(down=p + "0", up=p + "3")
    if k == N_LEVELS:
        return dict(down=p + "1", up=p + "3", upnorm=p + "4")
    return dict(down=p + "1", downnorm=p + "2", up=p + "5", upnorm=p + "6")


def gen_state_keys():
    """parameter names in registration order (= state_dict / .parameters() order)"""
    keys = [level_names(1)["down"] + ".weight"]
    for k in range(2, N_LEVELS):
        n = level_names(k)
        keys += [n["down"] + ".weight", n["downnorm"] + ".weight", n["downnorm"] + ".bias"]
    n = level_names(N_LEVELS)
    keys += [n["down"] + ".weight", n["up"] + ".weight", n["upnorm"] + ".weight", n["upnorm"] + ".bias"]
    for k in range(N_LEVELS - 1, 1, -1):
        n = level_names(k)
        keys += [n["up"] + ".weight", n["upnorm"] + ".weight", n["upnorm"] + ".bias"]
    n = level_names(1)
    keys += [n["up"] + ".weight", n["up"] + ".bias"]
    return keys


def gen_bucket_names():
    """the generator's gradient buckets in the order gen_backward completes them (parallel.FlatGrads)"""
    n1 = level_names(1)
    out = [[n1["up"] + ".weight", n1["up"] + ".bias"]]
    for k in range(2, N_LEVELS + 1):
        n = level_names(k)
        out.append([n["upnorm"] + ".weight", n["upnorm"] + ".bias", n["up"] + ".weight"])
    out.append([level_names(N_LEVELS)["down"] + ".weight"])
    for k in range(N_LEVELS - 1, 1, -1):
        n = level_names(k)
        out.append([n["downnorm"] + ".weight", n["downnorm"] + ".bias", n["down"] + ".weight"])
    out.append([n1["down"] + ".weight"])
    return out


DISC_CONVS = ["model.0", "model.2", "model.5", "model.8", "model.11"]
DISC_NORMS = {"model.2": "model.3", "model.5": "model.6", "model.8": "model.9"}
DISC_KEYS = ["model.0.weight", "model.0.bias", "model.2.weight", "model.3.weight", "model.3.bias", "model.5.weight",
             "model.6.weight", "model.6.bias", "model.8.weight", "model.9.weight", "model.9.bias", "model.11.weight",
             "model.11.bias"]


def disc_bucket_names():
    return [["model.11.weight", "model.11.bias"], ["model.9.weight", "model.9.bias", "model.8.weight"],
            ["model.6.weight", "model.6.bias", "model.5.weight"], ["model.3.weight", "model.3.bias", "model.2.weight"],
            ["model.0.weight", "model.0.bias"]]


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def dropout_shapes(n, h, w):
    """{level: NCHW shape of the tensor its Dropout applies to} at input h x w"""
    return {k: (n, 512, h >> (k - 1), w >> (k - 1)) for k in DROPOUT_LEVELS}


def draw_dropout(n, h, w, mode="host", device="cuda"):
    """One generator call's Dropout decisions: {level: device 0/1 mask} ("host": torch's CPU stream, regenerated
    on the device; the generator advanced before returning) or {level: seed} ("device")"""
    if mode == "host":
        masks, commit = draw_dropout_deferred(n, h, w, device)
        commit()
        return masks
    if mode != "device":
        raise ValueError(f"dropout mode must be 'device' or 'host' (got {mode!r})")
    base = int(torch.randint(1, 2 ** 62, (1,)).item())
    return {k: (_mix64(base + k) & 0x7FFFFFFFFFFFFFFF) or 1 for k in DROPOUT_LEVELS}


def dropout_masks(drop, n, h, w, device="cuda"):
    """{level: 0/1 mask} of a draw_dropout result (seeds materialised on the device; tests / inspection)"""
    out = {}
    for k, shape in dropout_shapes(n, h, w).items():
        d = drop[k]
        out[k] = ops.dropout_mask(d, shape, device) if isinstance(d, int) else d
    return out


def draw_dropout_deferred(n, h, w, device="cuda"):
    """"host" mode's masks as ({level: device 0/1 mask}, commit): commit() advances torch's CPU generator past
    the draw (the fused step calls it at its end: nothing else in the iteration draws from that generator)"""
    shapes = dropout_shapes(n, h, w)
    outs, commit = torch_rng.draw(list(shapes.values()), 1 - DROP_P, device)
    return dict(zip(shapes, outs)), commit


def draw_dropout_masks(n, h, w):
    """The Dropout masks of one generator call at input h x w, from torch's (CPU) global generator in
    the reference's CPU order: F.dropout draws empty_like(x).bernoulli_(1 - p) per call, levels 7, 6, 5.
    Returns {level: float32 0/1 mask [n, 512, h_k, w_k]} on the host."""
    masks = {}
    for k, shape in dropout_shapes(n, h, w).items():      # level k's up output = its input size
        masks[k] = torch.empty(shape, dtype=torch.float32).bernoulli_(1 - DROP_P)
    return masks


# ======================================================================================
# generator
# ======================================================================================

_conv_nb = conv_fwd          # (the name tests/test_gpu_unet_convs.py and tests/test_gpu_seg_train.py call it by)


def _convT4(P, name, X_, Y):
    """an up conv: ConvTranspose2d(k=4, s=2, p=1) over X_ (zero border >= 1)"""
    convT_fwd(P, name, X_, Y, 4, 1)


def check_input_size(H, W):
    if H < 256 or W < 256 or H % 256 or W % 256:
        raise RuntimeError(f"Pix2PixGenerator (U-Net-256) needs H, W multiples of 256 (got {H}x{W}): its eight "
                           "stride-2 levels and skip concatenations only line up there")


def gen_forward(P, B, x, masks=None, training=True, save=True):
    """x: [N, C, H, W] fp32 on the device (any strides); P: parameters, B: BatchNorm buffers (updated
    in place in training mode), masks: a draw_dropout result (training mode; drawn here, device mode,
    when None).  Returns (out [N, 3, H, W], saved)."""
    require_device(x, "generator input")
    N, Cin, H, W = x.shape
    check_input_size(H, W)
    dev = x.device
    if training and masks is None:
        masks = draw_dropout(N, H, W, device=x.device)
    dmask = {k: (m if isinstance(m, int) else m.to(dev)) for k, m in masks.items()} if training else {}
    ch = level_channels(Cin)
    S = dict(x=x, N=N, H=H, W=W, training=training, lv={})
    X0 = Buf.empty(N, H, W, PL.rup(Cin, 4), 1, dev)
    ops.pack_input(x, Cin, None, 0, X0, 0, N, FG_PAD_ZERO)
    a = X0                                             # level k's down-conv input
    for k in range(1, N_LEVELS + 1):
        nm = level_names(k)
        inner = ch[k - 1][1]
        h, w = H >> k, W >> k
        c = Buf.empty(N, h, w, inner, 0, dev)
        conv_fwd(P, nm["down"], a, 1, 4, 2, c)
        L = dict(a=a, c=c)
        if k == N_LEVELS:
            r = Buf.zeros(N, h, w, inner, 1, dev)
            ops.bn_apply(c, 1, None, None, None, None, None, FG_ACT_RELU, r)
            L["r"] = r
        else:
            mean = invstd = None
            if "downnorm" in nm:
                mean, invstd = bn_stats_for(B, nm["downnorm"], c, 1, training)
            nxt = Buf.zeros(N, h, w, inner, 1, dev)
            cat = Buf.zeros(N, h, w, 2 * inner, 1, dev)
            slot = ops.amax_slot(cat)               # one operand-scale slot, raised by both halves' producers
            gam = P.get(nm.get("downnorm", "") + ".weight")
            bet = P.get(nm.get("downnorm", "") + ".bias")
            ops.bn_apply(c, 1, mean, invstd, gam, bet, None, FG_ACT_LRELU, nxt, FG_ACT_RELU, Slice(cat, 0, inner),
                         slots=(None, slot))
            L.update(mean=mean, invstd=invstd, cat=cat, cat_slot=slot)
            a = nxt
        S["lv"][k] = L
    # up path, innermost first
    for k in range(N_LEVELS, 1, -1):
        nm = level_names(k)
        L = S["lv"][k]
        outer = ch[k - 1][2]
        h, w = H >> (k - 1), W >> (k - 1)
        u = Buf.empty(N, h, w, outer, 0, dev)
        _convT4(P, nm["up"], L["r"] if k == N_LEVELS else L["cat"], u)
        mean, invstd = bn_stats_for(B, nm["upnorm"], u, 1, training)
        parent = S["lv"][k - 1]
        inner_p = ch[k - 2][1]
        ops.bn_apply(u, 1, mean, invstd, P[nm["upnorm"] + ".weight"], P[nm["upnorm"] + ".bias"], dmask.get(k),
                     FG_ACT_RELU, Slice(parent["cat"], inner_p, inner_p), slots=(parent["cat_slot"], None))
        L.update(u=u, umean=mean, uinvstd=invstd, mask=dmask.get(k))
    nm = level_names(1)
    logits = Buf.empty(N, H, W, 4, 0, dev)
    _convT4(P, nm["up"], S["lv"][1]["cat"], logits)
    out = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
    ops.tanh_head_fwd(logits, 3, out)
    S["logits"] = logits
    return out, (S if save else None)


def gen_backward(P, S, g_out, grads_into=None, ready=None, accumulate=False):
    """Explicit backward of gen_forward (training-mode BatchNorm: through the batch statistics).
    g_out: [N, 3, H, W] (any strides).  Returns {parameter name: gradient}."""
    ready = ready or (lambda name: None)
    N, H, W = S["N"], S["H"], S["W"]
    dev = g_out.device
    G = Grads(P, grads_into, accumulate)
    ch = level_channels(S["x"].shape[1])
    lv = S["lv"]
    # ---- tanh head + outermost up conv (bias)
    nm = level_names(1)
    g_logits = Buf.empty(N, H, W, 4, 1, dev)
    ops.tanh_head_bwd(S["logits"], 3, g_out, g_logits)
    cat1 = lv[1]["cat"]
    g_cat = {1: Buf.empty(N, cat1.h, cat1.w, cat1.c, 0, dev)}
    convT_bwd(P, G, nm["up"], cat1, g_logits, 4, 1, g_cat[1], bias_channels=3)
    ready(nm["up"])
    # ---- up chain: level k's upnorm + up conv, k = 2 .. 8
    g_c = None
    for k in range(2, N_LEVELS + 1):
        nm = level_names(k)
        L = lv[k]
        outer, inner_p = ch[k - 1][2], ch[k - 2][1]
        u = L["u"]
        g_u = Buf.empty(N, u.h, u.w, outer, 1, dev)
        ops.bn_bwd(Slice(g_cat[k - 1], inner_p, inner_p), FG_ACT_RELU, None, 0, u, 1, L["umean"], L["uinvstd"],
                   P[nm["upnorm"] + ".weight"], P[nm["upnorm"] + ".bias"], L["mask"], g_u,
                   G.get(nm["upnorm"] + ".weight"), G.get(nm["upnorm"] + ".bias"), G.acc)
        ops.zero_border(g_u)
        xin = L["r"] if k == N_LEVELS else L["cat"]
        g_x = Buf.empty(N, xin.h, xin.w, xin.c, 0, dev)
        convT_bwd(P, G, nm["up"], xin, g_u, 4, 1, g_x)
        ready(nm["up"])
        if k == N_LEVELS:
            g_c = Buf.empty(N, xin.h, xin.w, xin.c, 1, dev)      # through ReLU(D_8)
            ops.bn_bwd(g_x, FG_ACT_RELU, None, 0, L["c"], 1, None, None, None, None, None, g_c)
            ops.zero_border(g_c)
        else:
            g_cat[k] = g_x
    # ---- down chain: level k's down conv (+ downnorm), k = 8 .. 2, then level 1
    for k in range(N_LEVELS, 1, -1):
        nm = level_names(k)
        L = lv[k]
        if k < N_LEVELS:
            inner = ch[k - 1][1]
            c = L["c"]
            g_c = Buf.empty(N, c.h, c.w, inner, 1, dev)
            ops.bn_bwd(g_a, FG_ACT_LRELU, Slice(g_cat[k], 0, inner), FG_ACT_RELU, c, 1, L["mean"], L["invstd"],
                       P[nm["downnorm"] + ".weight"], P[nm["downnorm"] + ".bias"], None, g_c,
                       G.get(nm["downnorm"] + ".weight"), G.get(nm["downnorm"] + ".bias"), G.acc)
            ops.zero_border(g_c)
        wgrad_conv(P, G, nm["down"], g_c, L["a"], 1, 4, 2)
        ready(nm["down"])
        a = L["a"]
        g_a = Buf.empty(N, a.h, a.w, a.c, 0, dev)
        dgrad_s2(P, nm["down"], g_c, 4, Y=g_a)
    L = lv[1]
    nm = level_names(1)
    g_d1 = Buf.empty(N, L["c"].h, L["c"].w, 64, 0, dev)
    ops.bn_bwd(g_a, FG_ACT_LRELU, Slice(g_cat[1], 0, 64), FG_ACT_RELU, L["c"], 1, None, None, None, None, None, g_d1)
    wgrad_conv(P, G, nm["down"], g_d1, L["a"], 1, 4, 2)
    ready(nm["down"])
    return G.out


def gen_act_decisions(S):
    """the generator's activation decisions in a saved forward, keyed by oracle/pix2pix.py's names
    (test instrumentation for teacher-forced gradient comparisons)"""
    lv = S["lv"]
    ch = level_channels(S["x"].shape[1])
    out = {"inner": decided(lv[N_LEVELS]["r"])}
    for k in range(1, N_LEVELS):
        out[f"down{k}"] = decided(lv[k + 1]["a"])
    for k in range(2, N_LEVELS + 1):
        inner_p = ch[k - 2][1]
        out[f"up{k}"] = decided(Slice(lv[k - 1]["cat"], inner_p, inner_p))
    return out


# ======================================================================================
# discriminator
# ======================================================================================

class DiscBatchNorm:
    """patchgan's norm object: BatchNorm2d (model.3 / .6 / .9) + LeakyReLU over `groups` separate calls stacked along
    the batch, B's running statistics updated in training mode; the convs under it have no bias"""

    conv_stats = False

    def __init__(self, B, groups, training):
        self.B, self.groups, self.training = B, groups, training

    def forward(self, P, conv, e, stats, fp32):
        norm = DISC_NORMS[conv]
        mean, invstd = bn_stats_for(self.B, norm, e, self.groups, self.training)
        a = Buf.zeros(e.n, e.h, e.w, e.c, 1, e.t.device)
        ops.bn_apply(e, self.groups, mean, invstd, P[norm + ".weight"], P[norm + ".bias"], None, FG_ACT_LRELU, a)
        return dict(e=e, mean=mean, invstd=invstd, a=a)

    def backward(self, P, G, conv, L, g_a, g_e):
        norm = DISC_NORMS[conv]
        gg, gb = (G.get(norm + ".weight"), G.get(norm + ".bias")) if G is not None else (None, None)
        ops.bn_bwd(g_a, FG_ACT_LRELU, None, 0, L["e"], self.groups, L["mean"], L["invstd"], P[norm + ".weight"],
                   P[norm + ".bias"], None, g_e, gg, gb)
        ops.zero_border(g_e)


def disc_forward(P, B, inp, groups=1, training=True, save=True):
    """inp: Buf from executor.disc_pack (zero border 1), groups: separate BatchNorm calls stacked
    along the batch.  Returns (pred [N, 1, ho, wo], saved)."""
    return patchgan.forward(P, inp, DiscBatchNorm(B, groups, training), save, "Pix2PixDiscriminator",
                            tags={"model.8": "p2p_d_model8_fwd"})


def disc_backward(P, S, g_pred, param_grads=True, grads_into=None, input_grad=None, input_grad_channels=None,
                  input_grad_accumulate=False, ready=None):
    """Explicit backward of disc_forward (patchgan.backward documents the arguments).  The restricted input gradient
    stays on the conv engine."""
    return patchgan.backward(P, S, g_pred, param_grads, grads_into, input_grad, input_grad_channels,
                             input_grad_accumulate, ready)


disc_act_decisions = patchgan.act_decisions
