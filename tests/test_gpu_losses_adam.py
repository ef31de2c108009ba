"""FusedAdam (fg_adam_step), LSGAN-MSE (fg_mse_const) and L1 (fg_l1) against float64 at the edges of their
launch geometry: more tensors than one launch holds, tensors around the block size, both lerp branches and
late steps of Adam; grid-striding past the block cap, a strided finalize, non-trivial strides, exact zeros
and accumulation for the losses.

Adam's measure is max|got - ref| / max|ref| per tensor (exp_avg and the update cancel, so a per-element
relative error is meaningless: torch's own fp32 Adam differs from fp64 by 1e-2 per element there).  The
bound, 2e-6, is set by the reference: torch's fp32 CPU Adam stays at or below 3e-7 by the same measure, and
every case asserts that it stays below 1e-6 on its own inputs."""
import pytest
import torch

from test_gpu_parity import DEV, conv_math  # noqa: F401  (conv_math is a fixture)

pytestmark = pytest.mark.gpu

ADAM_TOL = 2e-6          # fused kernel vs torch.optim.Adam in float64
ADAM_FP32_REF = 1e-6     # torch's own fp32 CPU Adam vs the same float64 run
LR = 2e-4

MAXT, EPB, SHARDS = 24, 2048, 64      # csrc/loss_adam.hip: tensors per launch, elements per block; absmax shards


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from floodgan import _lib as L
    L.check(L.load().fg_device_ok(), "device_ok")


def maxrel(got, ref):
    got, ref = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    if ref.numel() == 0:
        return 0.0 if got.numel() == 0 else float("inf")
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


class AdamTrio:
    """the same parameters under FusedAdam (device, fp32), torch.optim.Adam in float64 (the reference) and
    torch.optim.Adam in float32 (the measure of what fp32 can give), all on identical gradients"""

    def __init__(self, inits, **kw):
        from floodgan.optim import FusedAdam
        self.dev = [torch.nn.Parameter(w.clone().to(DEV)) for w in inits]
        self.r64 = [torch.nn.Parameter(w.double().clone()) for w in inits]
        self.r32 = [torch.nn.Parameter(w.clone()) for w in inits]
        self.od = FusedAdam(self.dev, **kw)
        self.o64 = torch.optim.Adam(self.r64, foreach=False, **kw)
        self.o32 = torch.optim.Adam(self.r32, foreach=False, **kw)

    def step(self, grads):
        """grads: one fp32 CPU tensor or None per parameter"""
        for ps, conv in ((self.dev, lambda g: g.clone().to(DEV)), (self.r64, lambda g: g.double()),
                         (self.r32, lambda g: g.clone())):
            for p, g in zip(ps, grads):
                p.grad = None if g is None else conv(g)
        self.od.step()
        self.o64.step()
        self.o32.step()
        torch.cuda.synchronize()

    def set_step(self, value):
        for opt in (self.od, self.o64, self.o32):
            for st in opt.state.values():
                st["step"].fill_(value)

    def errors(self, i):
        """(fused vs fp64, torch fp32 vs fp64), each {param, exp_avg, exp_avg_sq: max-norm relative error}"""
        out = []
        for ps, opt in ((self.dev, self.od), (self.r32, self.o32)):
            st, ref = opt.state[ps[i]], self.o64.state[self.r64[i]]
            out.append({"param": maxrel(ps[i], self.r64[i]), "exp_avg": maxrel(st["exp_avg"], ref["exp_avg"]),
                        "exp_avg_sq": maxrel(st["exp_avg_sq"], ref["exp_avg_sq"])})
        return out

    def check(self, what):
        """every tensor within ADAM_TOL of float64, torch's fp32 run within ADAM_FP32_REF; returns the worst"""
        worst = {"fused": 0.0, "torch_fp32": 0.0}
        for i in range(len(self.dev)):
            if self.r64[i] not in self.o64.state:
                assert self.dev[i] not in self.od.state, (what, i)
                continue
            fused, cpu32 = self.errors(i)
            print(f"{what} tensor {i} ({self.dev[i].numel()}): fused {fused} torch-fp32 {cpu32}")
            for k in fused:
                assert cpu32[k] < ADAM_FP32_REF, (what, i, k, cpu32[k])
                assert fused[k] < ADAM_TOL, (what, i, k, fused[k])
            assert float(self.od.state[self.dev[i]]["step"]) == float(self.o64.state[self.r64[i]]["step"]), (what, i)
            worst["fused"] = max(worst["fused"], *fused.values())
            worst["torch_fp32"] = max(worst["torch_fp32"], *cpu32.values())
        return worst


# 27 tensors: two launches (24 + 3).  Blocks of one element, a partial block, exactly one block, one block + 1
# element, two blocks + 1; the large one wraps the 64 absmax shards (66 blocks) and ends in a partial block,
# and sits in the second launch.
BIG = 64 * EPB + 2049
LAYOUT_SIZES = [1, 5, 2047, 2048, 2049, 4097, 6000, 3, 4096, 2050, 1, 1023, 6143, 2048, 7, 300, 4095, 2049, 64, 6145,
                1000, 2, 2048, 4099, 513, BIG, 2049]
LAST_IS_MAX = (4, 25)            # tensors whose largest |p| is their very last element: one per launch
assert len(LAYOUT_SIZES) == 27 > MAXT and LAYOUT_SIZES.index(BIG) >= MAXT and LAYOUT_SIZES.index(BIG) >= 27 - 3
assert LAST_IS_MAX[0] < MAXT <= LAST_IS_MAX[1] and (BIG + EPB - 1) // EPB > SHARDS and BIG % EPB


def _layout_scales():
    """one gradient scale per tensor over 1e-4 .. 1e2, neighbours 10^2.5 or more apart"""
    n = len(LAYOUT_SIZES)
    return [10.0 ** (-4 + 6 * ((11 * i) % n) / (n - 1)) for i in range(n)]


@pytest.mark.parametrize("init", ["zeros", "randn"])
@pytest.mark.parametrize("conv_math", ["fp32", "f16x3"], indirect=True)
def test_adam_tensor_layout(conv_math, init, report):
    """one FusedAdam over 27 parameters (two launches), three steps, every tensor's parameter / exp_avg /
    exp_avg_sq vs float64; under f16x3 the absmax slot the kernel raised is the parameter's exact max |p|"""
    from floodgan import ops
    g = torch.Generator().manual_seed(31)
    scales = _layout_scales()
    assert min(scales) == 1e-4 and max(scales) == pytest.approx(1e2)
    if init == "zeros":          # the update is seen at full fp32 precision
        inits = [torch.zeros(n) for n in LAYOUT_SIZES]
    else:
        inits = [torch.randn(n, generator=g) * 0.02 for n in LAYOUT_SIZES]
        for i in LAST_IS_MAX:
            inits[i][-1] = 1.0
    trio = AdamTrio(inits, lr=LR, betas=(0.5, 0.999))
    for step in range(3):
        trio.step([torch.randn(n, generator=g) * s for n, s in zip(LAYOUT_SIZES, scales)])
        worst = trio.check(f"layout/{conv_math}/{init}/step{step + 1}")
    report("adam_tensor_layout", conv_math=conv_math, init=init, **worst)
    for i, p in enumerate(trio.dev):
        slot = ops.slot_of(p)
        if conv_math != "f16x3":
            assert slot is None
            continue
        assert slot is not None and slot.numel() == SHARDS
        assert float(slot.max()) == float(p.detach().abs().max()), i
        assert ops.absmax(p) is slot, i
        if init == "randn" and i in LAST_IS_MAX:
            assert int(p.detach().abs().argmax()) == p.numel() - 1, i


@pytest.mark.parametrize("eps", [1e-8, 1e-3])
@pytest.mark.parametrize("betas", [(0.5, 0.999), (0.9, 0.999), (0.0, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("init", ["zeros", "randn"])
def test_adam_arithmetic(init, betas, eps, report):
    """both lerp forms (1 - beta1 below and above 0.5), beta1 = 0, a fast beta2, a large eps; steps 1, 2, 3 and
    step 1000 (the bias corrections close to 1)"""
    g = torch.Generator().manual_seed(int(1000 * betas[0]) + int(10 * betas[1]) + (eps > 1e-6))
    sizes, scales = [6000, 2049], [1.0, 1e-3]
    inits = [torch.zeros(n) if init == "zeros" else torch.randn(n, generator=g) * 0.02 for n in sizes]
    trio = AdamTrio(inits, lr=LR, betas=betas, eps=eps)
    worst = {}
    for step in (1, 2, 3, 1000):
        if step == 1000:
            trio.set_step(999)
        trio.step([torch.randn(n, generator=g) * s for n, s in zip(sizes, scales)])
        w = trio.check(f"arith/{init}/{betas}/{eps}/step{step}")
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
        assert float(trio.od.state[trio.dev[0]]["step"]) == step
    report("adam_arithmetic", init=init, betas=betas, eps=eps, **worst)


@pytest.mark.parametrize("betas", [(0.5, 0.999), (0.9, 0.999), (0.0, 0.999), (0.5, 0.9)])
def test_adam_lerp_after_gradient_collapse(betas, report):
    """the gradients shrink by 1e7 between two steps.  ATen's lerp takes end - (end - self) * (1 - w) for
    w >= 0.5 because self + w * (end - self) loses `end` beside a large `self`: at beta1 = 0 (w = 1) the new
    exp_avg is the gradient itself, which the other form would round away at the old exp_avg's ulp"""
    g = torch.Generator().manual_seed(41 + int(100 * betas[0]))
    sizes = [2049, 300]
    trio = AdamTrio([torch.zeros(n) for n in sizes], lr=LR, betas=betas)
    for step, scale in enumerate((1.0, 1e-7)):
        trio.step([torch.randn(n, generator=g) * scale for n in sizes])
        worst = trio.check(f"collapse/{betas}/step{step + 1}")
    if betas[0] == 0.0:
        for p, st in ((p, trio.od.state[p]) for p in trio.dev):
            assert torch.equal(st["exp_avg"], p.grad)
    report("adam_lerp_after_gradient_collapse", betas=betas, **worst)


@pytest.mark.parametrize("init", ["zeros", "randn"])
def test_adam_zero_gradient_first_step(init):
    """an all-zero gradient at step 1: 0 / (0 + eps) moves nothing; the state is finite (and zero)"""
    g = torch.Generator().manual_seed(3)
    inits = [torch.zeros(2049) if init == "zeros" else torch.randn(2049, generator=g) * 0.02, torch.randn(100, generator=g)]
    trio = AdamTrio(inits, lr=LR, betas=(0.5, 0.999))
    trio.step([torch.zeros(2049), torch.randn(100, generator=g)])
    assert torch.equal(trio.dev[0].detach().cpu(), inits[0])
    st = trio.od.state[trio.dev[0]]
    for k in ("exp_avg", "exp_avg_sq"):
        assert bool(torch.isfinite(st[k]).all()) and float(st[k].abs().max()) == 0.0
    assert torch.equal(trio.r64[0].detach(), inits[0].double())          # torch agrees
    fused, _ = trio.errors(1)
    assert max(fused.values()) < ADAM_TOL
    # and the next, non-zero step runs from that state like torch's
    trio.step([torch.randn(2049, generator=g), torch.randn(100, generator=g)])
    trio.check(f"zero-grad/{init}/step2")


def test_adam_by_step_grouping(report):
    """two of five parameters have no gradient on the first step and join on the second: FusedAdam groups the
    launches by step count, and every parameter's step matches torch's"""
    g = torch.Generator().manual_seed(17)
    sizes = [3000, 2049, 100, 4096, 7]
    late = (1, 3)
    trio = AdamTrio([torch.randn(n, generator=g) * 0.02 for n in sizes], lr=LR, betas=(0.9, 0.999))
    for step in range(3):
        trio.step([None if (step == 0 and i in late) else torch.randn(n, generator=g) * 10.0 ** (i - 2)
                   for i, n in enumerate(sizes)])
        worst = trio.check(f"by_step/step{step + 1}")
    for i in range(len(sizes)):
        want = 2.0 if i in late else 3.0
        assert float(trio.od.state[trio.dev[i]]["step"]) == want == float(trio.o64.state[trio.r64[i]]["step"])
    report("adam_by_step_grouping", **worst)


@pytest.mark.parametrize("conv_math", ["fp32", "f16x3"], indirect=True)
def test_adam_empty_parameter(conv_math):
    """torch.optim.Adam steps a group that holds an empty parameter; so does FusedAdam (ops.adam_step skips it:
    its data_ptr is null, which fg_adam_step rejects)"""
    from floodgan import ops
    g = torch.Generator().manual_seed(23)
    sizes = [100, 0, 2049]
    trio = AdamTrio([torch.randn(n, generator=g) * 0.02 for n in sizes], lr=LR, betas=(0.5, 0.999))
    for step in range(2):
        trio.step([torch.randn(n, generator=g) for n in sizes])
        trio.check(f"empty/{conv_math}/step{step + 1}")
    for opt, ps in ((trio.od, trio.dev), (trio.o64, trio.r64)):
        st = opt.state[ps[1]]
        assert float(st["step"]) == 2.0 and st["exp_avg"].numel() == 0 and st["exp_avg_sq"].numel() == 0
    # a call with nothing but empty entries launches nothing
    e = torch.empty(0, device=DEV)
    ops.adam_step([(e, e, e, e)], LR, 0.5, 0.999, 1e-8, 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ LSGAN-MSE

# 1 element; one block - 1 / + 1 element (blocks_for counts 1024 per block); 301 partials: mean_finalize's
# strided loop (> 256); 1026 blocks' worth: past the cap of 1024 blocks, so a fifth, ragged grid-stride pass
MSE_SIZES = [1, 1023, 1025, 300 * 1024 + 7, 1024 * 1024 + 1025]


@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse_const_vs_fp64(n, target, report):
    from floodgan import ops
    gen = torch.Generator().manual_seed(n % 9973 + int(target))
    p = torch.randn(n, generator=gen)
    gscale = 0.5
    pr = p.double()
    ref = float(((pr - target) ** 2).mean())
    gref = gscale * 2.0 * (pr - target) / n
    pd = p.to(DEV)
    out = torch.full((3,), float("nan"), device=DEV)
    grad = torch.full((n + 2,), float("nan"), device=DEV)
    ops.mse_const(pd, target, gscale, out[1:2], grad[1:n + 1])
    torch.cuda.synchronize()
    loss_err = abs(float(out[1]) - ref) / abs(ref)
    grad_err = maxrel(grad[1:n + 1], gref)
    print(f"mse n={n} target={target}: loss {float(out[1])!r} ref {ref!r} rel {loss_err:.2e}; grad {grad_err:.2e}")
    report("mse_const_vs_fp64", n=n, target=target, loss_rel=loss_err, grad_maxrel=grad_err)
    assert abs(float(out[1]) - ref) <= 1e-6 * abs(ref)
    assert grad_err < 1e-6
    assert bool(torch.isnan(out[[0, 2]]).all()) and bool(torch.isnan(grad[[0, n + 1]]).all())
    # g=None: the same loss, nothing else written
    out2 = torch.full((3,), float("nan"), device=DEV)
    ops.mse_const(pd, target, gscale, out2[1:2], None)
    torch.cuda.synchronize()
    assert float(out2[1]) == float(out[1]) and bool(torch.isnan(out2[[0, 2]]).all())
    assert torch.equal(pd.cpu(), p)


# ------------------------------------------------------------------ L1

@pytest.mark.parametrize("shape", [(3, 3, 7, 13), (2, 3, 419, 421)])       # the second: past 1024 blocks x 1024
def test_l1_strided_vs_fp64(shape, report):
    """a channels-last `a` against a channel slice `b` of a 9-channel tensor (every stride non-trivial), ~1% of the
    elements exactly equal: loss vs float64, the gradient bit for bit (+-fp32(gscale) / fp32(n) or 0; with
    accumulate the prior contents plus that, one fp32 addition)"""
    from floodgan import ops
    N, C, H, W = shape
    n = N * C * H * W
    gen = torch.Generator().manual_seed(H * W)
    a = torch.randn(shape, generator=gen)
    x = torch.randn((N, 9, H, W), generator=gen)
    same = torch.rand(shape, generator=gen) < 0.01
    x[:, 2:5][same] = a[same]
    assert 0 < int(same.sum()) <= n // 25
    ad =a.to(DEV).contiguous(memory_format=torch.channels_last)
    xd = x.to(DEV)
    bd = xd[:, 2:5]
    assert ad.stride() == (C * H * W, 1, W * C, C) and bd.stride() == (9 * H * W, H * W, W, 1)
    assert bd.data_ptr() != xd.data_ptr() and n < 2 ** 24
    b = x[:, 2:5]
    ref = float((a.double() - b.double()).abs().mean())
    gscale = 100.0
    gs = torch.tensor(gscale, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    sg = torch.sign(a - b) * gs                                     # fp32; 0 where equal
    assert int((sg == 0).sum()) == int(same.sum())
    out = torch.full((3,), float("nan"), device=DEV)
    grad = torch.full(shape, float("nan"), device=DEV)
    ops.l1(ad, bd, gscale, out[1:2], grad)
    torch.cuda.synchronize()
    l1v = float(out[1])
    err = abs(l1v - ref) / ref
    print(f"l1 {shape}: loss {l1v!r} ref {ref!r} rel {err:.2e}; {int(same.sum())} equal elements")
    report("l1_strided_vs_fp64", shape=list(shape), loss_rel=err, equal=int(same.sum()))
    assert abs(l1v - ref) <= 1e-6 * abs(ref)
    assert grad.is_contiguous() and torch.equal(grad.cpu(), sg)
    assert bool(torch.isnan(out[[0, 2]]).all())
    # accumulate onto existing contents
    prior = torch.randn(shape, generator=gen) * float(gs) * 3
    grad2 = prior.to(DEV)
    ops.l1(ad, bd, gscale, out[1:2], grad2, accumulate=True)
    torch.cuda.synchronize()
    assert float(out[1]) == l1v and torch.equal(grad2.cpu(), prior + sg)
    # g=None writes the loss alone; loss_scale is one fp32 product of the mean
    out3 = torch.full((3,), float("nan"), device=DEV)
    ops.l1(ad, bd, gscale, out3[1:2], None, loss_scale=100.0)
    torch.cuda.synchronize()
    assert float(out3[1]) == float(torch.tensor(l1v, dtype=torch.float32) * 100.0)
    assert bool(torch.isnan(out3[[0, 2]]).all())
    assert torch.equal(ad.cpu(), a) and torch.equal(xd.cpu(), x)
