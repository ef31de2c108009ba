"""The layout kernels (csrc/layout.hip: fg_pack_input, fg_zero_border, fg_fold_add, fg_unfold_nchw) and the output
heads (csrc/tail.hip: fg_tanh_head_fwd / _bwd, fg_tail_fwd / _bwd) at their edges, against torch-CPU references:
F.pad + torch.cat bit for bit where a kernel only copies or zeroes, fp64 (autograd for the adjoints) within both
forms of the kernel bound (test_gpu_bnorm.close) where it computes.  Sources carry NaN wherever a kernel must not
read (borders, channels above the valid count) and every output starts as NaN, so a stale read, an unwritten
element and a write outside the stated region all fail."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_bnorm import NAN, buf_nan_border, close, f16x3, nan_buf  # noqa: F401  (f16x3: a fixture)
from test_gpu_parity import DEV, _fold_cpu, nchw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def border_is_zero(B):
    """the border of B is exactly 0 (a NaN left there fails)"""
    t, p = B.nhwc().cpu().clone(), B.pad
    t[:, p:p + B.h, p:p + B.w] = 0.0
    return bool((t == 0).all())


# ------------------------------------------------------------------ fg_pack_input

def _pack_ref(a, ca, b, cb, c_alloc, pad, mode):
    """F.pad(torch.cat(...)) in fp32, NHWC over the padded extent; the channels above ca + cb are zero"""
    n, _, h, w = a.shape
    parts = [a[:, :ca]] + ([b[:, :cb]] if cb else []) + [torch.zeros(n, c_alloc - ca - cb, h, w)]
    x = torch.cat(parts, 1)
    if pad:
        x = F.pad(x, (pad,) * 4, mode="reflect" if mode else "constant")
    return x.permute(0, 2, 3, 1).contiguous()


# c_alloc <= 16 takes the per-pixel kernel (float4 stores when c_alloc % 4 == 0, scalar stores at 6: reachable through
# the C ABI only), 32 the generic element-per-thread kernel
PACK_CASES = [(4, 3, 0), (12, 9, 3), (12, 3, 6), (16, 9, 7), (6, 3, 2), (32, 20, 5)]


@pytest.mark.parametrize("c_alloc,ca,cb", PACK_CASES)
def test_pack_input(c_alloc, ca, cb):
    """zero and reflect padding at pad 0, 1 and 3; (12, 3, 6) and (6, 3, 2) leave zero channels"""
    from floodgan import ops
    g = _gen(c_alloc * 100 + ca)
    n, h, w = 2, 7, 9
    a, b = torch.randn(n, ca, h, w, generator=g), torch.randn(n, max(cb, 1), h, w, generator=g)
    ad, bd = a.to(DEV), (b.to(DEV) if cb else None)
    for mode in (0, 1):
        for pad in (0, 1, 3):
            dst = nan_buf(n, h, w, c_alloc, pad)
            ops.pack_input(ad, ca, bd, cb, dst, 0, n, mode)
            torch.cuda.synchronize()
            assert torch.equal(dst.nhwc().cpu(), _pack_ref(a, ca, b, cb, c_alloc, pad, mode)), (mode, pad)


def test_pack_input_generic_past_grid_cap():
    """2 x 257 x 257 x 32 = 4,227,136 elements exceed the generic kernel's 16384 x 256 = 4,194,304 threads"""
    from floodgan import ops
    g = _gen(31)
    n, h, w, pad = 2, 251, 251, 3
    a, b = torch.randn(n, 20, h, w, generator=g), torch.randn(n, 5, h, w, generator=g)
    dst = nan_buf(n, h, w, 32, pad)
    ops.pack_input(a.to(DEV), 20, b.to(DEV), 5, dst, 0, n, 1)
    torch.cuda.synchronize()
    assert torch.equal(dst.nhwc().cpu(), _pack_ref(a, 20, b, 5, 32, pad, 1))


@pytest.mark.parametrize("c_alloc", [4, 32])
def test_pack_input_reflect_limits(c_alloc):
    """reflect at the smallest legal size (pad = h - 1); pad >= h is refused and nothing is written"""
    from floodgan import ops
    g = _gen(32)
    a = torch.randn(2, 3, 4, 5, generator=g)
    dst = nan_buf(2, 4, 5, c_alloc, 3)
    ops.pack_input(a.to(DEV), 3, None, 0, dst, 0, 2, 1)
    torch.cuda.synchronize()
    assert torch.equal(dst.nhwc().cpu(), _pack_ref(a, 3, None, 0, c_alloc, 3, 1))
    for h, w in ((3, 5), (5, 3)):
        dst = nan_buf(2, h, w, c_alloc, 3)
        with pytest.raises(RuntimeError, match="reflect pad"):
            ops.pack_input(torch.randn(2, 3, h, w, generator=g).to(DEV), 3, None, 0, dst, 0, 2, 1)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dst.t).all())


@pytest.mark.parametrize("c_alloc", [12, 32])
def test_pack_input_source_forms(c_alloc):
    """a channels-last view, a channel slice x[:, 2:5] and a width-strided view x[..., ::2] as sources"""
    from floodgan import ops
    g = _gen(33)
    n, h, w = 2, 6, 7
    cl = torch.randn(n, h, w, 5, generator=g).to(DEV).permute(0, 3, 1, 2)             # channels last
    wide = torch.randn(n, 8, h, w, generator=g).to(DEV)
    strided = torch.randn(n, 4, h, 2 * w, generator=g).to(DEV)
    for a, ca, b, cb in ((cl, 5, wide[:, 2:5], 3), (wide[:, 2:5], 3, strided[..., ::2], 4),
                         (strided[..., ::2], 4, cl, 5)):
        assert not a.is_contiguous() and not b.is_contiguous()
        for mode, pad in ((0, 1), (1, 3)):
            dst = nan_buf(n, h, w, c_alloc, pad)
            ops.pack_input(a, ca, b, cb, dst, 0, n, mode)
            torch.cuda.synchronize()
            assert torch.equal(dst.nhwc().cpu(), _pack_ref(a.cpu(), ca, b.cpu(), cb, c_alloc, pad, mode))


@pytest.mark.parametrize("c_alloc", [12, 32])
def test_pack_input_image_range(c_alloc):
    """img0 = 1, nimg = 2 into a 4-image destination: source images 0, 1 land in 1, 2; images 0 and 3 stay NaN"""
    from floodgan import ops
    g = _gen(34)
    a, b = torch.randn(2, 9, 5, 6, generator=g), torch.randn(2, 3, 5, 6, generator=g)
    dst = nan_buf(4, 5, 6, c_alloc, 2)
    ops.pack_input(a.to(DEV), 9, b.to(DEV), 3, dst, 1, 2, 1)
    torch.cuda.synchronize()
    out = dst.nhwc().cpu()
    assert torch.equal(out[1:3], _pack_ref(a, 9, b, 3, c_alloc, 2, 1))
    assert bool(torch.isnan(out[0]).all()) and bool(torch.isnan(out[3]).all())


def test_pack_input_wide_row():
    """w = 300 (302 padded): the per-pixel kernel's second block in x"""
    from floodgan import ops
    g = _gen(35)
    a = torch.randn(1, 3, 3, 300, generator=g)
    for mode in (0, 1):
        dst = nan_buf(1, 3, 300, 4, 1)
        ops.pack_input(a.to(DEV), 3, None, 0, dst, 0, 1, mode)
        torch.cuda.synchronize()
        assert torch.equal(dst.nhwc().cpu(), _pack_ref(a, 3, None, 0, 4, 1, mode))


@pytest.mark.parametrize("c_alloc,h,w", [(12, 7, 300), (32, 7, 9)])
def test_pack_input_absmax_slot(f16x3, c_alloc, h, w):
    """the slot a full pack raises equals the maximum of what was written (zero border: the largest source
    value sits in the last image's corner and is written once)"""
    from floodgan import ops
    g = _gen(36)
    a, b = torch.randn(2, 3, h, w, generator=g), torch.randn(2, 6, h, w, generator=g)
    b[1, 5, h - 1, w - 1] = -77.0
    for mode in (0, 1):
        dst = nan_buf(2, h, w, c_alloc, 2)
        ops.pack_input(a.to(DEV), 3, b.to(DEV), 6, dst, 0, 2, mode)
        torch.cuda.synchronize()
        assert float(ops.slot_of(dst).max()) == float(dst.t.abs().max()) == 77.0


# ------------------------------------------------------------------ fg_zero_border

def _zero_border_case(n, h, w, c, pad, seed):
    from floodgan import ops
    from floodgan.plans import Buf
    g = _gen(seed)
    t = torch.randn(n, h + 2 * pad, w + 2 * pad, c, generator=g)
    inside = torch.zeros(n, h + 2 * pad, w + 2 * pad, 1, dtype=torch.bool)
    inside[:, pad:pad + h, pad:pad + w] = True
    t = torch.where(~inside & (torch.rand(t.shape, generator=g) < 0.5), torch.full_like(t, NAN), t)   # NaN and values
    B = Buf(t.reshape(-1).to(DEV), n, h, w, c, pad)
    ops.zero_border(B)
    torch.cuda.synchronize()
    assert torch.equal(B.nhwc().cpu(), torch.where(inside, t, torch.zeros_like(t)))


@pytest.mark.parametrize("pad", [0, 1, 3, 6])
@pytest.mark.parametrize("h,w", [(7, 5), (16, 16)])
def test_zero_border(h, w, pad):
    """afterwards the border is exactly 0 and the interior bit-identical; pad 0 changes nothing"""
    for c in (4, 64):
        _zero_border_case(3, h, w, c, pad, 40 + pad)


def test_zero_border_past_grid_cap():
    """16 x (2 * 6 * 28 + 2 * 6 * 16) x 256 = 2,162,688 border elements exceed the kernel's 8192 x 256 = 2,097,152
    threads: a second grid-stride iteration"""
    _zero_border_case(16, 16, 16, 256, 6, 47)


# ------------------------------------------------------------------ fg_fold_add

# (C, destination pad, add's pad or None for no add, gpad's own pad)
FOLD_FORMS = [(4, 0, None, 0), (64, 1, 3, 2), (256, 3, 0, 1), (64, 0, 1, 0)]


@pytest.mark.parametrize("small", [True, False])
@pytest.mark.parametrize("fold", [0, 1, 3])
def test_fold_add(fold, small, report):
    """the adjoint of reflect padding plus `add`; at (fold + 1) x (fold + 2) a row has three pre-images (fold < h
    at its limit); the destination border is written as exactly 0"""
    from floodgan import ops
    n = 2
    h, w = (fold + 1, fold + 2) if small else (13, 17)
    for c, dpad, apad, gpad_pad in FOLD_FORMS:
        g = _gen(50 + fold + c)
        gp = torch.randn(n, c, h + 2 * fold, w + 2 * fold, generator=g).double()
        add = torch.randn(n, c, h, w, generator=g).double() if apad is not None else None
        ref = _fold_cpu(gp, fold) if fold else gp.clone()
        if add is not None:
            ref = ref + add
        dst = nan_buf(n, h, w, c, dpad)
        ops.fold_add(buf_nan_border(gp, gpad_pad), fold, None if add is None else buf_nan_border(add, apad), dst)
        torch.cuda.synchronize()
        close(f"fold_add fold{fold} {h}x{w} c{c}", nchw(dst), ref, report)
        assert border_is_zero(dst)


# ------------------------------------------------------------------ fg_unfold_nchw

# (N, H, W, fold, c, acc_channels); the last has 2 x 12 x 420 x 420 = 4,233,600 elements, above the kernel's
# 16384 x 256 = 4,194,304 threads
UNFOLD_CASES = [(1, 2, 3, 1, 4, 0), (1, 4, 5, 3, 9, 3), (2, 4, 5, 3, 12, 0), (1, 1, 2, 0, 3, 3), (2, 13, 17, 3, 9, 3),
                (2, 420, 420, 3, 12, 3)]


@pytest.mark.parametrize("N,H,W,p,c,acc", UNFOLD_CASES)
def test_unfold_nchw_edges(N, H, W, p, c, acc, report):
    """into a strided NCHW destination: channels < acc accumulate, the others start as NaN and are overwritten, the
    destination's channel c (beyond the unfolded ones) stays NaN"""
    from floodgan import ops
    from floodgan.plans import Buf
    g = _gen(60 + H + c)
    gpad = torch.randn(N, c, H + 2 * p, W + 2 * p, generator=g)
    ref = _fold_cpu(gpad.double(), p) if p else gpad.double()
    G = buf_nan_border(gpad, 0, (c + 3) // 4 * 4)
    base = torch.randn(N, c + 1, H, W, generator=g)
    base[:, acc:] = NAN
    dst = base.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)   # non-contiguous NCHW view
    ops.unfold_nchw(G, p, c, dst, acc_channels=acc)
    torch.cuda.synchronize()
    ref[:, :acc] += base[:, :acc].double()
    close(f"unfold_nchw {N}x{c}x{H}x{W} fold{p}", dst[:, :c], ref, report)
    assert bool(torch.isnan(dst[:, c]).all())


# ------------------------------------------------------------------ fg_tanh_head_fwd / _bwd

def _head_logits(n, c, h, w, scale, g):
    if scale == 20:     # every |logit| in [20, 40): tanh is +-1 and its derivative exactly 0 in fp32
        x = (20 + 20 * torch.rand(n, c, h, w, generator=g)) * (torch.randint(0, 2, (n, c, h, w), generator=g) * 2 - 1)
    else:
        x = torch.randn(n, c, h, w, generator=g) * scale
    return x.float().double()


@pytest.mark.parametrize("H,W", [(1, 1), (16, 16), (19, 300)])
@pytest.mark.parametrize("c_alloc", [4, 64])
def test_tanh_head(c_alloc, H, W, report):
    """c = 3 of c_alloc logit channels (NaN in the others and in the logits' border: nothing may leak); out and
    g_out are the first three channels of 4-channel tensors, NCHW and channels-last (their fourth channel must stay /
    is NaN); g_logits (pad 3) gets an exactly zero border and exactly zero channels >= 3"""
    from floodgan import ops
    n, c = 2, 3
    g = _gen(70 + H + c_alloc)
    for pad in (0, 3):
        for scale in (1e-4, 1.0, 20):
            for chlast in (False, True):
                x = _head_logits(n, c, H, W, scale, g)
                go = torch.randn(n, c, H, W, generator=g).double()
                logits = buf_nan_border(x, pad, c_alloc)
                shape4 = (n, H, W, 4) if chlast else (n, 4, H, W)
                out4, g4 = torch.full(shape4, NAN, device=DEV), torch.full(shape4, NAN, device=DEV)
                if chlast:
                    out4, g4 = out4.permute(0, 3, 1, 2), g4.permute(0, 3, 1, 2)
                g4[:, :3] = go.float().to(DEV)
                tag = f"tanh_head c_alloc{c_alloc} {H}x{W} pad{pad} scale{scale:g}"
                ops.tanh_head_fwd(logits, c, out4[:, :3])
                torch.cuda.synchronize()
                close(tag + " fwd", out4[:, :3], torch.tanh(x), report)
                assert bool(torch.isnan(out4[:, 3]).all())
                gl = nan_buf(n, H, W, c_alloc, 3)
                ops.tanh_head_bwd(logits, c, g4[:, :3], gl)
                torch.cuda.synchronize()
                ref = go * (1 - torch.tanh(x) ** 2)
                if scale == 20:
                    assert float(ref.abs().max()) < 1e-15 and bool((gl.t == 0).all())
                else:
                    close(tag + " bwd", nchw(gl, c), ref, report)
                assert bool((gl.nhwc()[..., c:] == 0).all()) and border_is_zero(gl)


# ------------------------------------------------------------------ fg_tail_fwd / _bwd

def _tail_ref(cl, al, x):
    t, a = torch.tanh(cl), torch.softmax(al, 1)
    out = sum(t[:, 3 * i:3 * i + 3] * a[:, i:i + 1] for i in range(9)) + x[:, :3] * a[:, 9:10]
    return out, a


# name: (N, H, W, content logits, attention logits, cl c_alloc, al c_alloc, logits' pad, x form, g_content c_alloc / pad)
TAIL_CASES = {
    # attention spread +-80 (the max-subtracted softmax; underflowed weights are 0, not NaN), content +-15 (tanh
    # saturates), the smallest allocations with NaN in cl channel 27 and al channels 10, 11
    "spread": (2, 16, 16, "pm15", "pm80", 28, 12, 2, "chlast", 64, 0),
    # all ten attention logits of a pixel equal (at -100, 0 or 100): every weight is 0.1
    "equal": (2, 19, 300, "n01", "equal", 32, 16, 0, "c3", 32, 6),
    "one_pixel": (1, 1, 1, "n01", "n01", 28, 12, 2, "c3", 64, 0),
    "one_pixel_equal": (1, 1, 1, "pm15", "equal", 32, 12, 0, "chlast", 32, 1),
}


@pytest.mark.parametrize("name", list(TAIL_CASES))
def test_tail_edges(name, report):
    from floodgan import ops
    N, H, W, ckind, akind, cca, aca, lpad, xform, gca, gpad = TAIL_CASES[name]
    g = _gen(80 + H)
    cl = torch.randn(N, 27, H, W, generator=g) if ckind == "n01" else (torch.rand(N, 27, H, W, generator=g) * 2 - 1) * 15
    if akind == "n01":
        al = torch.randn(N, 10, H, W, generator=g)
    elif akind == "pm80":
        al = (torch.rand(N, 10, H, W, generator=g) * 2 - 1) * 80
    else:
        al = ((torch.randint(0, 3, (N, 1, H, W), generator=g) - 1) * 100.0).expand(N, 10, H, W).contiguous()
    xc = 3 if xform == "c3" else 9
    x = torch.randn(N, xc, H, W, generator=g)
    go, gm = torch.randn(N, 3, H, W, generator=g), torch.randn(N, H, W, generator=g)
    clr, alr = (t.double().requires_grad_(True) for t in (cl, al))
    out, a = _tail_ref(clr, alr, x.double())
    gcl_ref, gal_ref = torch.autograd.grad((out, a[:, 9]), (clr, alr), (go.double(), gm.double()))

    CL, AL = buf_nan_border(cl, lpad, cca), buf_nan_border(al, lpad, aca)
    xd = x.to(DEV)
    if xform == "chlast":
        xd = xd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    o, mk = torch.full((N, 3, H, W), NAN, device=DEV), torch.full((N, H, W), NAN, device=DEV)
    ops.tail_fwd(CL, AL, xd, o, mk)
    torch.cuda.synchronize()
    close(f"tail {name} out", o, out, report)
    close(f"tail {name} mask", mk, a[:, 9], report)
    if akind == "equal":
        assert bool((mk == torch.tensor(0.1, dtype=torch.float32)).all())

    GC, GA = nan_buf(N, H, W, gca, gpad), nan_buf(N, H, W, 16, 0)
    ops.tail_bwd(CL, AL, xd, go.to(DEV), GC, GA, g_mask=gm.to(DEV))
    torch.cuda.synchronize()
    close(f"tail {name} g_content", nchw(GC, 27), gcl_ref, report)
    close(f"tail {name} g_att", nchw(GA, 10), gal_ref, report)
    assert bool((GC.nhwc()[..., 27:] == 0).all()) and border_is_zero(GC)
    assert bool((GA.nhwc()[..., 10:] == 0).all())
