"""The flood-mask loss without a device (floodgan.segmentation.FloodMaskLoss and its kernels' wrappers): exports,
defaults, and the refusals every entry point makes before it reaches the library."""
import pytest
import torch


def test_exports_and_defaults():
    import floodgan
    from floodgan import _lib as L
    from floodgan import ops
    from floodgan.model import PairedStep, Pix2PixStep
    from floodgan.segmentation import FloodMaskLoss, UNet
    assert floodgan.FloodMaskLoss is FloodMaskLoss and "FloodMaskLoss" in floodgan.__all__
    for name in ("fg_bn_bwd_fixed", "fg_flood_mask_bce", "fg_unit_image_bwd"):
        assert name in L.SIGNATURES, name
    for name in ("bn_bwd_fixed", "flood_mask_bce", "unit_image_bwd"):
        assert callable(getattr(ops, name)), name
    assert UNet.input_grad is False and UNet().input_grad is False
    assert PairedStep.fake_loss is None and Pix2PixStep.fake_loss is None


def test_unet_backward_keywords_default_to_todays_call():
    import inspect

    from floodgan import segmentation as S
    sig = inspect.signature(S.unet_backward)
    assert list(sig.parameters) == ["P", "S", "g_logits", "grads_into", "choices", "input_grad", "param_grads"]
    assert sig.parameters["input_grad"].default is False and sig.parameters["param_grads"].default is True
    assert sig.parameters["input_grad"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(S.unet_logits).parameters["update_running"].default is True


def test_entry_points_reject_cpu_tensors():
    from floodgan import ops
    from floodgan.plans import Buf
    from floodgan.segmentation import FloodMaskLoss, UNet
    msg = "must be a float32 tensor on a HIP device"
    x = torch.zeros(1, 3, 16, 16)
    loss = FloodMaskLoss(UNet())
    with pytest.raises(RuntimeError, match=msg):
        loss(x, x)
    with pytest.raises(RuntimeError, match=msg):
        loss.logits(x, x)
    with pytest.raises(RuntimeError, match=msg):
        loss.fused_term(0.25)(x, x, torch.zeros_like(x), 0.25)
    net = UNet()
    net.input_grad = True
    with pytest.raises(RuntimeError, match=msg):
        net(x.clone().requires_grad_(True))
    b4, b8 = Buf.zeros(1, 16, 16, 4, 0, "cpu"), Buf.zeros(1, 16, 16, 8, 0, "cpu")
    c = torch.ones(8)
    with pytest.raises(RuntimeError, match=msg):
        ops.bn_bwd_fixed(b8, 1, None, 0, b8, c, c, c, c, b8)
    with pytest.raises(RuntimeError, match=msg):
        ops.flood_mask_bce(b4, b4, 1.0, b4, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=msg):
        ops.unit_image_bwd(b4, x, torch.zeros_like(x))


def test_flood_mask_loss_takes_a_unet_only():
    from floodgan.segmentation import FloodMaskLoss, UNet
    with pytest.raises(TypeError, match="UNet"):
        FloodMaskLoss(torch.nn.Conv2d(3, 1, 1))
    with pytest.raises(NotImplementedError):
        FloodMaskLoss(UNet(bilinear=True))
    loss = FloodMaskLoss(UNet(), batch_stats=True)
    assert loss.batch_stats is True and isinstance(loss.seg, UNet)
    with pytest.raises(RuntimeError, match="before any call"):
        loss.read()


def test_model_needs_a_segmentation_path_for_the_term():
    from floodgan.model import Model
    with pytest.raises(ValueError, match="segmentation_model_path"):
        Model(model="PairedAttention", device="cpu", flood_mask_weight=0.25)
    with pytest.raises(ValueError, match="flood_mask_weight"):
        Model(model="PairedAttention", device="cpu", flood_mask_weight=-1.0)
    with pytest.raises(NotImplementedError, match="paired step"):
        Model(model="CycleGAN", device="cpu", flood_mask_weight=0.25, segmentation_model_path="seg.pth.tar")
    m = Model(model="PairedAttention", device="cpu")
    assert m.flood_mask_weight == 0.0 and len(m.paired_loss_keys()) == 4
    assert list(m.all_losses) == ["all_" + k for k in m.paired_loss_keys()]
    m = Model(model="PairedAttention", device="cpu", flood_mask_weight=0.25, segmentation_model_path="seg.pth.tar")
    assert m.paired_loss_keys()[4] == "losses_flood_mask_generator_synthetic"
    assert list(m.all_losses)[4] == "all_losses_flood_mask_generator_synthetic"
