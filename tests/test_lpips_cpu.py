"""LPIPS on the CPU: the weight loader's layouts and failures, the fp64 oracle's basic properties, and a sensitivity
guard in the style of test_oracle_sensitivity.py -- each way the formula could be misread moves the oracle's value
on the GPU tests' inputs by at least 100x the bound the GPU tests hold the HIP path to, so those tests would catch
it."""
import pytest
import torch

import lpips_oracle as LO
from floodgan.evaluate import LPIPS_SCALE, LPIPS_SHIFT, load_lpips_weights, lpips_weight_shapes


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_loader_layouts_agree(tmp_path):
    sd = LO.weights()
    ref = load_lpips_weights(sd)
    assert {k: tuple(v.shape) for k, v in ref.items()} == lpips_weight_shapes()
    assert all(v.dtype == torch.float32 and v.device.type == "cpu" for v in ref.values())
    assert torch.equal(ref["conv2.weight"], sd["net.slice2.3.weight"])
    assert torch.equal(ref["lin3.weight"], sd["lin3.model.1.weight"].flatten())
    with_scaling = dict(sd)
    with_scaling["scaling_layer.shift"] = torch.tensor(LPIPS_SHIFT).view(1, 3, 1, 1)
    with_scaling["scaling_layer.scale"] = torch.tensor(LPIPS_SCALE).view(1, 3, 1, 1)
    wrapped = {"net." + k: v for k, v in with_scaling.items()}                  # a metric's state_dict()
    module = dict(sd)
    module.update({f"lins.{k}.model.1.weight": sd[f"lin{k}.model.1.weight"] for k in range(5)})
    for other in (with_scaling, wrapped, LO.parts_layout(sd), module, ref):
        assert _same(load_lpips_weights(other), ref)
    path = tmp_path / "alex.pth"
    torch.save(wrapped, path)
    assert _same(load_lpips_weights(str(path)), ref)
    assert _same(load_lpips_weights(path), ref)
    # the result is a copy: editing the source afterwards does not reach it
    sd["net.slice1.0.bias"] += 1
    assert not torch.equal(ref["conv1.bias"], sd["net.slice1.0.bias"])


@pytest.mark.parametrize("layout", ["lpips", "wrapped", "parts"])
def test_loader_failures_name_the_key(layout):
    def make():
        sd = LO.weights()
        return {"lpips": sd, "wrapped": {"net." + k: v for k, v in sd.items()}, "parts": LO.parts_layout(sd)}[layout]

    conv_key = {"lpips": "net.slice3.6.bias", "wrapped": "net.slice3.6.bias", "parts": "features.6.bias"}[layout]
    pre = "net." if layout == "wrapped" else ""
    sd = make()
    del sd[pre + conv_key]
    with pytest.raises(ValueError, match=conv_key.replace(".", r"\.")):
        load_lpips_weights(sd)
    sd = make()
    del sd[pre + "lin4.model.1.weight"]
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight"):
        load_lpips_weights(sd)
    sd = make()
    sd[pre + conv_key] = sd[pre + conv_key][:-1]
    with pytest.raises(ValueError, match=conv_key.replace(".", r"\.")):
        load_lpips_weights(sd)
    sd = make()
    sd[pre + "lin1.model.1.weight"] = sd[pre + "lin1.model.1.weight"].flatten()       # [C] instead of [1, C, 1, 1]
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        load_lpips_weights(sd)
    sd = make()
    sd[pre + "classifier.1.weight"] = torch.zeros(3)
    with pytest.raises(ValueError, match=r"unexpected key 'classifier\.1\.weight'"):
        load_lpips_weights(sd)
    for key, const in (("scaling_layer.shift", LPIPS_SHIFT), ("scaling_layer.scale", LPIPS_SCALE)):
        sd = make()
        sd[pre + key] = torch.tensor(const).view(1, 3, 1, 1) + torch.tensor([0.0, 1e-4, 0.0]).view(1, 3, 1, 1)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            load_lpips_weights(sd)
    with pytest.raises(ValueError):
        load_lpips_weights({})


@pytest.mark.parametrize("case", LO.E2E_CASES)
def test_oracle_zero_and_symmetric(case):
    a, b = LO.e2e_inputs(*case)
    sd = LO.seeded_weights()
    assert torch.equal(LO.lpips(a, a, sd), torch.zeros(case[0], dtype=torch.float64))
    ab, ba = LO.lpips(a, b, sd), LO.lpips(b, a, sd)
    assert (ab > 0).all() and torch.allclose(ab, ba, rtol=1e-12, atol=0)
    assert torch.equal(ab, LO.e2e_reference(*case)[0])


@pytest.mark.parametrize("case", LO.E2E_CASES)
def test_oracle_sensitivity_end_to_end(case):
    """omitting the scaling layer, padding before the scaling, or dropping any one tap each moves every image's
    value by >= 100x the end-to-end bound of the GPU test on the same inputs"""
    a, b = LO.e2e_inputs(*case)
    sd = LO.seeded_weights()
    ref, bound = LO.e2e_reference(*case)[0], float(LO.e2e_bound(*case).max())
    assert 0 < LO.e2e_fp32_error() < 1e-5                             # the yardstick is an fp32-rounding figure
    moved = {"no scaling layer": LO.lpips(a, b, sd, scaling=False),
             "pad before scaling": LO.lpips(a, b, sd, pad_after_scaling=False)}
    moved.update({f"tap {k} dropped": LO.lpips(a, b, sd, drop_tap=k) for k in range(5)})
    for what, val in moved.items():
        shift = float((val - ref).abs().min())
        print(f"lpips sensitivity {case} {what}: moves by {shift:.3e} = {shift / bound:.1e} x the bound {bound:.2e}")
        assert shift >= 100 * bound, (what, shift, bound)


def test_oracle_sensitivity_eps_form():
    """f / (n + eps) instead of f / sqrt(eps + n^2) on the layer tests' inputs with dead and nearly dead pixels
    (no image in [0, 1] makes a whole 64-vector of seeded-weight features vanish, so this guard runs on the tap
    inputs): image 0 of every case from 3 x 5 up moves by >= 100x the layer bound and the end-to-end bounds"""
    bound = LO.layer_bound()
    assert 0 < bound <= 1e-6
    e2e = max(float(LO.e2e_bound(*c).max()) for c in LO.E2E_CASES)
    for case in LO.LAYER_CASES:
        f0, f1, lw = LO.layer_inputs(*case)
        ref = LO.layer_reference(*case)
        assert ref[1] == 0 and ref[0] > 0
        other = LO.layer_distance(f0, f1, lw, eps_form="add")
        assert other[1] == 0
        if case[1] * case[2] > 2:
            shift = float((other[0] - ref[0]).abs())
            print(f"lpips eps-form sensitivity {case}: moves by {shift:.3e}, relative {shift / float(ref[0]):.1e}")
            assert shift >= 100 * bound * float(ref[0]) and shift >= 100 * e2e, (case, shift, bound, e2e)


def test_layer_oracle_matches_the_formula_by_hand():
    """d_k on a 1 x 1 map, written out"""
    f0 = torch.tensor([3.0, 0.0, 4.0]).view(1, 3, 1, 1)
    f1 = torch.tensor([0.0, 2.0, 0.0]).view(1, 3, 1, 1)
    w = torch.tensor([0.5, 2.0, 1.0])
    n0, n1 = (1e-8 + 25.0) ** 0.5, (1e-8 + 4.0) ** 0.5
    want = 0.5 * (3 / n0) ** 2 + 2.0 * (2 / n1) ** 2 + 1.0 * (4 / n0) ** 2
    assert float(LO.layer_distance(f0, f1, w)[0]) == pytest.approx(want, rel=1e-14)
