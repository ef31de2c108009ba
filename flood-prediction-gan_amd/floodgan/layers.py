"""The layer kit the executors (floodgan.executor, floodgan.patchgan, floodgan.pix2pix, floodgan.segmentation) are
written with: the destination of parameter gradients, and the conv / transposed-conv forward, weight-gradient and
input-gradient launches over NHWC buffers (floodgan.plans.Buf), each a plan from floodgan.plans handed to
floodgan.ops.  Nothing here knows a network.
"""
import torch

from . import _lib as L
from . import ops
from . import plans as PL
from ._lib import FG_ACT_NONE
from .plans import Buf


class Grads:
    """Destination of parameter gradients: either fresh tensors (autograd path) or
    preallocated .grad tensors (fused step).

    Every launch runs on the caller's (current) stream.  Weight gradients on a second stream beside the
    input-gradient chain were measured slower (profiles/round2/r2m_*: 57.3 vs 56.6 ms per step; the
    pipelined convs already hold every CU, so the overlapped kernels each slow down by the same factor)
    and that path was removed in round 5."""

    def __init__(self, params, into=None, accumulate=False):
        self.params, self.into = params, into
        self.acc = accumulate       # raise existing gradients (a network used several times per step)
        self.out = {}

    def get(self, name):
        if name not in self.out:
            p = self.params[name]
            if self.into is not None and name in self.into:
                self.out[name] = self.into[name]
            else:
                self.out[name] = torch.empty_like(p)
        return self.out[name]

    def wgrad(self, prob, wmap, name, tag=None):
        ops.wgrad(prob, wmap, self.get(name), accumulate=self.acc, tag=tag)


def conv_fwd(P, name, X, pad, k, stride, Y, act=FG_ACT_NONE, tag=None, in_stats=False):
    """conv (its module may have no bias: bias=False in the reference).  Returns the InstanceNorm statistics of Y
    from the conv's epilogue when in_stats and available"""
    w = P[name + ".weight"]
    m = PL.wmap_conv_fwd(w.shape, X.c)
    return ops.conv([PL.conv_problem(X, pad, k, stride, ops.pack_weight(w, m), m, Y, bias=P.get(name + ".bias"),
                                     act=act)], tag=tag, in_stats=in_stats)


# round 5: the four output phases of a stride-2, 3-tap transposed op with 64 output channels as ONE problem (the quad
# form, plans.quad_map): each input pixel gathered once for all phases, zero segments skipped in the kernel.  The
# FLOODGAN_QUAD=0 switch was retired in round 6: the four-phase problems remain for every other shape, and
# tests/test_gpu_parity.py::test_quad_convT checks the quad form against fp64.
def quad_ok(X, shape, k, Y):
    return (k == 3 and shape[1] == 64 and isinstance(Y, Buf) and Y.c == 64 and ops.is_presplit(X)
            and L.fwd_f16x3() and (Y.h, Y.w, Y.n) == (2 * X.h, 2 * X.w, X.n) and X.pad >= 1 and X.c % 32 == 0
            and X.c & (X.c - 1) == 0)


def quad(P, name, X, Y, bias=None, in_stats=False):
    w = P[name + ".weight"]
    m, d0, mask = PL.quad_map(w.shape, 3, 1, X.c)
    return ops.conv([PL.quad_problem(X, m, d0, mask, ops.pack_weight(w, m), Y, bias=bias)], in_stats=in_stats)


def convT_fwd(P, name, X, Y, k, pad, in_stats=False):
    """ConvTranspose2d(k, stride 2, padding pad) over X (zero border >= 1) into Y (Buf or Slice), bias fused where
    the module has one: four sub-pixel phase GEMMs (k=2: one tap each), or the quad form where it applies (k=3,
    pad 1).  Returns what conv_fwd returns"""
    w = P[name + ".weight"]
    bias = P.get(name + ".bias")
    if pad == 1 and quad_ok(X, w.shape, k, Y):
        return quad(P, name, X, Y, bias=bias, in_stats=in_stats)
    maps = PL.phase_maps(w.shape, k, pad, X.c)
    wps = [ops.pack_weight(w, m) for m, _, _ in maps]
    return ops.conv(PL.phase_problems(X, w.shape, k, pad, Y, wps, maps, bias=bias), in_stats=in_stats)


def wgrad_conv(P, G, name, gy, X, pad, k, stride, tag=None):
    w = P[name + ".weight"]
    G.wgrad(PL.wgrad_conv(gy, X, pad, k, stride, w.shape[0]), PL.wmap_wgrad(w.shape, True, X.c, k), name + ".weight",
            tag=tag)


def dgrad_s1(P, name, gyp, pad_used, k, Y):
    w = P[name + ".weight"]
    m = PL.wmap_conv_dgrad_s1(w.shape, gyp.c)
    ops.conv([PL.conv_problem(gyp, pad_used, k, 1, ops.pack_weight(w, m), m, Y)])


def dgrad_s2(P, name, gy, k, Y=None, y_nchw=None, n_base=0, n_out=None, accumulate=0):
    w = P[name + ".weight"]
    if y_nchw is None and not n_base and n_out is None and not accumulate and quad_ok(gy, w.shape, k, Y):
        quad(P, name, gy, Y)
        return
    maps = PL.phase_maps(w.shape, k, 1, gy.c, n_base=n_base, n_out=n_out)
    wps = [ops.pack_weight(w, m) for m, _, _ in maps]
    ops.conv(PL.phase_problems(gy, w.shape, k, 1, Y, wps, maps, y_nchw=y_nchw, accumulate=accumulate))


def convT_bwd(P, G, name, xin, gy, k, pad, Y, accumulate=0, param_grads=True, bias_channels=None):
    """Backward of convT_fwd (weight (I, O, k, k)) from its output gradient gy (zero border >= pad; k=2: none needed,
    the four taps tile the output): the weight gradient into G, then the gradient of the input xin into Y (written,
    or += with accumulate) as one stride-2 GEMM with K = k * k * O.  bias_channels: also the bias gradient, as the
    channel sums of gy's first bias_channels channels (a layer whose bias no norm backward accounts for).
    param_grads=False: the input gradient only, and xin is not read"""
    w = P[name + ".weight"]
    if param_grads:
        G.wgrad(PL.wgrad_convT(xin, gy, k, pad, w.shape[0]), PL.wmap_wgrad(w.shape, True, gy.c, k), name + ".weight")
        if bias_channels is not None:
            ops.channel_sum(gy, bias_channels, G.get(name + ".bias"), G.acc)
    m = PL.wmap_convT_dgrad(w.shape, gy.c)
    ops.conv([PL.conv_problem(gy, pad, k, 2, ops.pack_weight(w, m), m, Y, accumulate=accumulate)])


def bn_stats_for(B, name, src, groups, training):
    """BatchNorm statistics (mean, invstd) of src: batch statistics (+ the update of B's running statistics, once
    per group) or, in eval mode, the running statistics"""
    rm, rv = B[name + ".running_mean"], B[name + ".running_var"]
    if training:
        return ops.bn_stats(src, groups, (rm, rv, B.get(name + ".num_batches_tracked")))
    mean, invstd = ops.bn_eval_stats(rm, rv)
    if groups > 1:
        mean, invstd = mean.repeat(groups), invstd.repeat(groups)
    return mean, invstd


def decided(B, lo=0, hi=None, pre=None, mean=None):
    """activation decisions of an activation-output Buf (output > 0 <=> input > 0 for ReLU and
    LeakyReLU): NCHW bool on the host.  A pre-split output (FG_PRESPLIT) is decided from the norm's input
    `pre` and `mean` instead: act((c - mean) * rstd) > 0 <=> c > mean (rstd > 0; fp32 subtraction keeps the
    sign)."""
    if B is None or ops.is_presplit(B) or ops.is_splitpix(B):     # (None: the fused head's unwritten activation)
        d = pre.interior() > mean.view(pre.n, 1, 1, pre.c)
        return d[lo:hi].permute(0, 3, 1, 2).contiguous().cpu()
    return (B.interior()[lo:hi] > 0).permute(0, 3, 1, 2).contiguous().cpu()
