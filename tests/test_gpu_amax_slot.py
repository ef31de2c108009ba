"""Every kernel that raises an absmax slot (csrc/amax_slot.hpp), under the f16x3 math, at two launch geometries.

A producer that measures its output must leave exactly max |storage| in the slot: the maximum of |values| is exact and
order-independent, so equality is the criterion and there is no tolerance.  A producer that publishes a bound instead
(pre-split and split-pixels outputs) must leave a slot that bounds the values its pieces decode to, and no h piece
above 2^14.

"big": more blocks than the slot has shards (64), with one planted extreme where the last block, its last wave and
its last lane see it -- N = 2, 40 x 16, 64 channels, border 1 (84 blocks of the row kernels, 95 of the grid-stride
ones); pack_input with 9 channels and border 3; the generator tail, whose channel counts are fixed and whose threads
walk pixels, at 96 x 80 (78 blocks).  "small": fewer blocks than shards and mostly idle blocks -- N = 1, 8 x 8, 4
channels (8 for the pre-split formats, 32 for split pixels and 64 for the fused head: the least those kernels take).
Each case also asserts that the extreme did land where it was aimed."""
import functools

import pytest
import torch

from test_gpu_bnorm import NAN, f16x3, nan_buf  # noqa: F401  (f16x3: a fixture)
from test_gpu_parity import DEV, _decode_presplit, buf_from

pytestmark = pytest.mark.gpu

BIG, SMALL = "big", "small"
GEOM = {BIG: (2, 40, 16, 64), SMALL: (1, 8, 8, 4)}      # N, H, W, C
PEAK = 77.0


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def geom(g, c_min=4):
    n, h, w, c = GEOM[g]
    return n, h, w, max(c, c_min)


@functools.lru_cache(maxsize=None)
def unit(n, c, h, w, seed=0):
    """unit-scale NCHW data, made once per shape (callers clone before planting)"""
    return torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(100 + seed))


def planted(n, c, h, w, y, x, seed=0, value=PEAK, ch=-1):
    t = unit(n, c, h, w, seed).clone()
    t[-1, ch, y, x] = value
    return t


def measured(dst, pixel=None):
    """the slot of dst holds exactly max |storage|; pixel (y, x in the padded extent of the last image): the maximum
    sits there"""
    from floodgan import ops
    torch.cuda.synchronize()
    t = ops._tensor(dst)
    top = float(t.abs().max())
    assert top > 0 and float(ops.slot_of(dst).max()) == top
    if pixel is not None:
        assert float(dst.nhwc()[-1, pixel[0], pixel[1]].abs().max()) == top


def bounded(slot, decoded, h_pieces):
    torch.cuda.synchronize()
    top = float(decoded.abs().max())
    assert top > 0 and float(slot.max()) >= top
    assert float(h_pieces.abs().float().max()) <= 2.0 ** 14


def presplit_bounded(B):
    from floodgan import ops
    assert ops.is_presplit(B)
    torch.cuda.synchronize()
    dec, _ = _decode_presplit(B, ops.slot_of(B))
    bounded(ops.slot_of(B), dec, B.t.view(torch.float16).view(-1, 2, 8)[:, 0])


def splitpix_bounded(B):
    """fg_split_pixels layout (include/floodgan.h): per pixel the 16-B chunks [h(C) | l(C)], chunk k of the pixel in
    padded column x stored at k ^ swz_pixel(x) (csrc/conv_common.hpp)"""
    import math
    from floodgan import ops
    assert ops.is_splitpix(B)
    torch.cuda.synchronize()
    slot = ops.slot_of(B)
    s = 2.0 ** (14 - math.frexp(float(slot.max()))[1])
    hp, wp, nch = B.h + 2 * B.pad, B.w + 2 * B.pad, B.c // 4
    t = B.t.view(torch.float16).view(B.n, hp, wp, nch, 8).cpu()
    xs = torch.arange(wp)
    swz = ((xs & 7) << 1) if B.c == 64 else (((xs >> 1) & 3) << 1)
    at = torch.arange(nch)[None, :] ^ swz[:, None]                   # [wp, nch]: where chunk k of column x is stored
    t = torch.gather(t, 3, at[None, None, :, :, None].expand(B.n, hp, wp, nch, 8))
    h, l = t[:, :, :, :nch // 2].double(), t[:, :, :, nch // 2:].double()
    bounded(slot, (h + l) / s, h)


# ------------------------------------------------------------------ the producers

def run_absmax(g):
    """65 blocks, the last one partly filled; the extreme in the last whole quad (the last block's last working lane)
    and, in a second tensor, in the unaligned tail after it"""
    from floodgan import ops
    n = 64 * 1024 + 4 * 200 + 3 if g == BIG else 7
    for at in (n - n % 4 - 1, n - 1):
        t = unit(1, 1, 1, n).flatten().clone()
        t[at] = -PEAK
        t = t.to(DEV)
        slot = ops.absmax(t)
        torch.cuda.synchronize()
        assert float(slot.max()) == float(t.abs().max()) == PEAK


def _pack(g, c_alloc, ca, cb, parts):
    """reflect padding, border 3: the storage ends with the reflection of interior pixel (H - 4, W - 4)"""
    from floodgan import ops
    n, h, w, _ = geom(g)
    pad = 3
    a = unit(parts * n, ca, h, w, 1).to(DEV)
    b = planted(parts * n, cb, h, w, h - 1 - pad, w - 1 - pad, 2, -PEAK).to(DEV)
    dst = nan_buf(parts * n, h, w, c_alloc, pad)
    if parts == 1:
        ops.pack_input(a, ca, b, cb, dst, 0, n, 1)
    else:
        slot = ops.amax_slot(dst)
        for i in range(parts):
            ops.pack_input(a[i * n:(i + 1) * n], ca, b[i * n:(i + 1) * n], cb, dst, i * n, n, 1, amax=slot)
    measured(dst, (-1, -1))
    assert float(dst.t[-1]) == -PEAK


def run_pack_input(g):
    _pack(g, 9 if g == BIG else 4, 6 if g == BIG else 3, 3 if g == BIG else 1, 1)      # one thread per pixel
    _pack(g, 32, 20, 12, 1)                                                            # one thread per element


def run_pack_input_parts(g):
    _pack(g, 9 if g == BIG else 4, 6 if g == BIG else 3, 3 if g == BIG else 1, 2)


def _norm_src(g, c_min=4, y=-2, x=-2, value=PEAK):
    """a conv output with one spike (its normalised value is the largest of the buffer) and its statistics"""
    from floodgan import ops
    n, h, w, c = geom(g, c_min)
    src = buf_from(planted(n, c, h, w, y, x, 3, value), 0, "constant")
    return (n, h, w, c), src, ops.in_stats(src)


def _in_apply(g):
    """reflect border 1: the storage ends with the reflection of interior pixel (H - 2, W - 2)"""
    from floodgan import ops
    (n, h, w, c), src, (mean, rstd) = _norm_src(g)
    dst = nan_buf(n, h, w, c, 1)
    ops.in_apply(src, mean, rstd, 0, None, dst, 1)
    measured(dst, (-1, -1))


def _grid_stride(fn, g):
    from floodgan import _lib as L
    lib = L.load()
    assert lib.fg_set_in_rows(0) == 0
    try:
        fn(g)
    finally:
        lib.fg_set_in_rows(1)


def run_in_apply_rows(g):
    _in_apply(g)


def run_in_apply_grid(g):
    _grid_stride(_in_apply, g)


def run_in_apply_ps_copy(g):
    """the fp32 dst is measured (the residual carries the extreme), the pre-split copy publishes a bound"""
    from floodgan import ops
    (n, h, w, c), src, (mean, rstd) = _norm_src(g, 8, 0, 0)
    res = buf_from(planted(n, c, h, w, -2, -2, 4, -PEAK), 0, "constant")
    dst, ps = nan_buf(n, h, w, c, 1), nan_buf(n, h, w, c, 1)
    ops.in_apply(src, mean, rstd, 1, res, dst, 1, ps_copy=ps)
    measured(dst, (-1, -1))
    presplit_bounded(ps)


def run_in_apply_head(g):
    from floodgan import ops
    from floodgan.plans import Buf
    (n, h, w, c), src, (mean, rstd) = _norm_src(g, 64, -1, -1)
    gen = torch.Generator().manual_seed(5)
    wt, b = (torch.randn(10, 64, generator=gen) * 0.1).to(DEV), torch.randn(10, generator=gen).to(DEV)
    dst, Y = nan_buf(n, h, w, c, 0), Buf.empty(n, h, w, 16, 0, DEV)
    ops.in_apply_head(src, mean, rstd, 0, dst, 0, wt, b, 10, Y)
    measured(dst, (-1, -1))


def _in_bwd(g):
    """the gradient's extreme at the last interior pixel; dst has a zero border"""
    from floodgan import ops
    (n, h, w, c), src, (mean, rstd) = _norm_src(g, 4, 0, 0, 0.5)
    gsrc = buf_from(planted(n, c, h, w, -1, -1, 6), 0, "constant")
    dst = nan_buf(n, h, w, c, 1)
    ops.in_bwd(gsrc, 0, None, src, mean, rstd, 0, dst)
    measured(dst, (-2, -2))


def run_in_bwd_rows(g):
    _in_bwd(g)


def run_in_bwd_grid(g):
    _grid_stride(_in_bwd, g)


def run_act_bwd(g):
    from floodgan import _lib as L
    from floodgan import ops
    n, h, w, c4 = geom(g)
    for c in (c4, 3):                                       # the float4 kernel; the element-per-thread kernel
        gb = buf_from(planted(n, c, h, w, -1, -1, 7, -PEAK), 1, "constant")
        yb = buf_from(planted(n, c, h, w, -1, -1, 8, 1.0), 1, "constant")
        ops.act_bwd(gb, yb, L.FG_ACT_LRELU, border_zero=True)
        measured(gb, (-2, -2))
        assert float(gb.nhwc()[-1, -2, -2, -1]) == -PEAK


def _bn(g):
    """two spikes at the last pixel: -77 in the last channel (the largest |u|, cut by ReLU) and 8 in the one before
    (the largest positive u); gamma = 1, beta = 0"""
    from floodgan import ops
    n, h, w, c = geom(g)
    x = planted(n, c, h, w, -1, -1, 9, -PEAK)
    x[-1, -2, -1, -1] = 8.0
    src = buf_from(x, 0, "constant")
    return (n, h, w, c), src, ops.bn_stats(src, 1), torch.ones(c, device=DEV), torch.zeros(c, device=DEV)


def run_bn_apply(g):
    """two destinations of different maxima raised by one launch: ReLU into a whole buffer, no activation into a
    channel slice of a wider one with a slot of its own"""
    from floodgan import _lib as L
    from floodgan import ops
    from floodgan.plans import Slice
    (n, h, w, c), src, (mean, invstd), gamma, beta = _bn(g)
    d0, wide = nan_buf(n, h, w, c, 0), nan_buf(n, h, w, 2 * c, 0)
    slot = ops.amax_slot(wide)
    ops.bn_apply(src, 1, mean, invstd, gamma, beta, None, L.FG_ACT_RELU, d0, L.FG_ACT_NONE, Slice(wide, c, c),
                 slots=(None, slot))
    measured(d0, (-1, -1))
    m0, m1 = float(d0.t.abs().max()), float(wide.interior()[..., c:].abs().max())
    assert m1 > m0 > 0 and ops.slot_of(wide) is slot and float(slot.max()) == m1
    assert float(wide.interior()[-1, -1, -1, -1].abs()) == m1 and float(d0.t[-2]) == m0


def _bn_bwd(g, fixed):
    from floodgan import _lib as L
    from floodgan import ops
    n, h, w, c = geom(g)
    src = buf_from(planted(n, c, h, w, -1, -1, 10, 3.0), 0, "constant")      # the last element's ReLU gate is open
    mean, invstd = ops.bn_stats(src, 1)
    gamma, beta = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    gA = buf_from(planted(n, c, h, w, -1, -1, 11), 0, "constant")
    dst = nan_buf(n, h, w, c, 0)
    if fixed:
        ops.bn_bwd_fixed(gA, L.FG_ACT_RELU, None, 0, src, mean, invstd, gamma, beta, dst)
    else:
        ops.bn_bwd(gA, L.FG_ACT_RELU, None, 0, src, 1, mean, invstd, gamma, beta, None, dst)
    measured(dst, (-1, -1))
    assert float(dst.t[-1].abs()) == float(dst.t.abs().max())


def run_bn_bwd(g):
    _bn_bwd(g, False)


def run_bn_bwd_fixed(g):
    _bn_bwd(g, True)


def run_tail_bwd(g):
    """both slots of one launch; the output gradient's extreme at the last pixel makes both gradients largest there"""
    from floodgan import ops
    from floodgan.plans import Buf
    n, h, w = (2, 96, 80) if g == BIG else (1, 8, 8)
    CL = buf_from(unit(n, 27, h, w, 12) * 0.5, 0, "constant", 32)
    AL = buf_from(unit(n, 10, h, w, 13), 0, "constant", 16)
    x = unit(n, 9, h, w, 14).to(DEV)
    gout = planted(n, 3, h, w, -1, -1, 15, 1e4).to(DEV)
    GC, GA = Buf.empty(n, h, w, 32, 6, DEV), Buf.empty(n, h, w, 16, 0, DEV)
    GC.t.fill_(NAN)
    GA.t.fill_(NAN)
    ops.tail_bwd(CL, AL, x, gout, GC, GA)
    measured(GC, (-7, -7))
    measured(GA, (-1, -1))


def run_adam(g):
    """one parameter of 64 blocks and one element: the last block holds one element, and it ends largest"""
    from floodgan import ops
    from floodgan.optim import FusedAdam
    n = 64 * 2048 + 1 if g == BIG else 4
    init = unit(1, 1, 1, n, 16).flatten() * 0.02
    init[-1] = 0.1
    grad = unit(1, 1, 1, n, 17).flatten().clone()
    grad[-1] = -PEAK                                        # the step raises the last element further
    p = torch.nn.Parameter(init.to(DEV))
    p.grad = grad.to(DEV)
    FusedAdam([p], lr=2e-4, betas=(0.5, 0.999)).step()
    torch.cuda.synchronize()
    slot = ops.slot_of(p)
    assert slot is not None and float(slot.max()) == float(p.detach().abs().max()) == float(p.detach()[-1]) > 0.1


def run_in_apply_presplit(g):
    from floodgan import ops
    (n, h, w, c), src, (mean, rstd) = _norm_src(g, 8)
    ps = nan_buf(n, h, w, c, 1)
    ops.in_apply(src, mean, rstd, 1, None, ps, 1, presplit=True)
    presplit_bounded(ps)


def run_in_apply_splitpix(g):
    from floodgan import ops
    (n, h, w, c), src, (mean, rstd) = _norm_src(g, 64 if g == BIG else 32)
    sp = nan_buf(n, h, w, c, 1)
    ops.in_apply(src, mean, rstd, 1, None, sp, 1, splitpix=True)
    splitpix_bounded(sp)


def run_in_bwd_presplit(g):
    from floodgan import ops
    (n, h, w, c), src, (mean, rstd) = _norm_src(g, 8, 0, 0, 0.5)
    gsrc = buf_from(planted(n, c, h, w, -1, -1, 6), 0, "constant")
    gp = nan_buf(n, h, w, c, 1)
    ops.in_bwd(gsrc, 0, None, src, mean, rstd, 0, gp, presplit=True)
    presplit_bounded(gp)


PRODUCERS = [run_absmax, run_pack_input, run_pack_input_parts, run_in_apply_rows, run_in_apply_grid,
             run_in_apply_ps_copy, run_in_apply_head, run_in_bwd_rows, run_in_bwd_grid, run_act_bwd, run_bn_apply,
             run_bn_bwd, run_bn_bwd_fixed, run_tail_bwd, run_adam,
             run_in_apply_presplit, run_in_apply_splitpix, run_in_bwd_presplit]


@pytest.mark.parametrize("g", [BIG, SMALL])
@pytest.mark.parametrize("producer", PRODUCERS, ids=[p.__name__[4:] for p in PRODUCERS])
def test_slot_raised(f16x3, producer, g):
    producer(g)
