"""CPU oracle of the segmentation U-Net's training step (checker only; tests/test_seg_train_oracle_golden.py pins it
to the reference's own SegmentationModel.train_model).

A functional restatement of models/model_architectures.py:508-587 and models/segmentation_model.py:65-67, 250-277:
conv, training-mode F.batch_norm, ReLU, 2x2 max-pool, conv_transpose2d, cat, binary_cross_entropy_with_logits,
torch.optim.Adam(1e-4, (0.5, 0.999)) under the LambdaLR of lambda_rule -- in any dtype.

Teacher forcing (oracle.paired_attention.ActDecisions is the model).  Two fp32 evaluations decide a ReLU whose input
sits within rounding of 0, or a max-pool window whose two largest values sit within rounding of each other,
differently, and one flip moves the gradients of a whole network.  To compare gradients, the oracle takes the
implementation's decisions: Decisions(relu={BatchNorm name: bool NCHW}, pool={"pool<k>": window position 0..3 per
pooled element, NCHW}).  Every forced layer logs (kind, name, disagreements, the largest distance from the kink over
them, relative to the layer's rms): the caller asserts that every disagreement sits at the kink.
"""
import torch
import torch.nn.functional as F

ENC = ["inc"] + [f"down{k}.maxpool_conv.1" for k in range(1, 5)]
DEC = [f"up{k}" for k in range(1, 5)]
LR, BETAS = 1e-4, (0.5, 0.999)


def lambda_rule(epoch, num_epochs):
    """models/segmentation_model.py:86-92"""
    return 1.0 - max(0, epoch + 1 - (num_epochs / 2)) / float((num_epochs / 2) + 1)


class Decisions:
    def __init__(self, relu=None, pool=None):
        self.relu, self.pool = relu or {}, pool or {}
        self.log = []

    def worst(self):
        """largest normalised distance from the kink at which a decision differed (0 if none)"""
        return max([w for _, _, n, w in self.log if n] or [0.0])

    def differing(self):
        return sum(n for _, _, n, _ in self.log)


def _relu(h, name, dec):
    if dec is None or name not in dec.relu:
        return F.relu(h)
    m = dec.relu[name].to(h.device).contiguous()         # contiguous NCHW (see oracle.paired_attention._act)
    hd = h.detach()
    dis = (hd > 0) != m
    n = int(dis.sum())
    rms = float(hd.pow(2).mean().sqrt()) or 1.0
    dec.log.append(("relu", name, n, float(hd[dis].abs().max()) / rms if n else 0.0))
    return torch.where(m, h, h * 0)


def _windows(x):
    """[N, C, h/2, w/2, 4]: each 2x2 window in the scan order (0,0), (0,1), (1,0), (1,1)"""
    N, C, H, W = x.shape
    return x.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)


def first_max(x):
    """ATen's max_pool2d choice per window: the first maximum in the scan order"""
    w = _windows(x)
    eq = w == w.max(-1, keepdim=True).values
    first = eq & (eq.cumsum(-1) == 1)
    return (first * torch.arange(4, device=x.device)).sum(-1)


def _pool(x, name, dec):
    if dec is None or name not in dec.pool:
        return F.max_pool2d(x, 2)
    idx = dec.pool[name].to(x.device).long().contiguous()
    w = _windows(x)
    out = w.gather(-1, idx.unsqueeze(-1)).squeeze(-1)
    xd = x.detach()
    dis = first_max(xd) != idx
    n = int(dis.sum())
    rms = float(xd.pow(2).mean().sqrt()) or 1.0
    gap = (_windows(xd).max(-1).values - out.detach())[dis]
    dec.log.append(("pool", name, n, float(gap.abs().max()) / rms if n else 0.0))
    return out.contiguous()


def _bn(P, B, name, h, training):
    nbt = B.get(name + ".num_batches_tracked")
    if training and nbt is not None:
        nbt += 1
    return F.batch_norm(h, B[name + ".running_mean"], B[name + ".running_var"], P[name + ".weight"], P[name + ".bias"],
                        training, 0.1, 1e-5)


def _double_conv(P, B, prefix, x, training, dec):
    c1, b1, c2, b2 = (f"{prefix}.double_conv.{i}" for i in (0, 1, 3, 4))
    h = _relu(_bn(P, B, b1, F.conv2d(x, P[c1 + ".weight"], None, padding=1), training), b1, dec)
    return _relu(_bn(P, B, b2, F.conv2d(h, P[c2 + ".weight"], None, padding=1), training), b2, dec)


def unet_forward(P, B, x, training=True, decisions=None):
    """logits [N, 1, H, W] of UNet(3, 1, bilinear=False); B's running statistics are updated in place in training
    mode (H, W multiples of 16: Up's size padding is then the identity)"""
    skips = []
    h = x
    for k, prefix in enumerate(ENC):
        if k:
            h = _pool(h, f"pool{k - 1}", decisions)
        h = _double_conv(P, B, prefix, h, training, decisions)
        skips.append(h)
    for i, up in enumerate(DEC):
        h = F.conv_transpose2d(h, P[up + ".up.weight"], P[up + ".up.bias"], stride=2)
        h = _double_conv(P, B, up + ".conv", torch.cat([skips[3 - i], h], dim=1), training, decisions)
    return F.conv2d(h, P["outc.conv.weight"], P["outc.conv.bias"])


def convT2_grads(x, w, b, g):
    """(input, weight, bias) gradients of F.conv_transpose2d(x, w, b, stride=2) under the output gradient g"""
    x, w, b = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    return torch.autograd.grad(F.conv_transpose2d(x, w, b, stride=2), (x, w, b), g)


class SegStepOracle:
    """The training iteration of models/segmentation_model.py:261-274 from a module's state
    (named_parameters / named_buffers, e.g. floodgan.segmentation.UNet on the CPU: same keys as the reference)."""

    def __init__(self, module, dtype=torch.float32, num_epochs=100):
        self.dtype, self.num_epochs = dtype, num_epochs
        self.P = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in module.named_parameters()}
        self.B = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()).clone()
                  for k, v in module.named_buffers()}
        self.opt = torch.optim.Adam(list(self.P.values()), lr=LR, betas=BETAS)
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, lr_lambda=lambda e: lambda_rule(e, self.num_epochs))

    def load_optimizer(self, state_dict):
        """continue from another Adam's state (same parameter order), converted to this oracle's dtype"""
        sd = {"state": {i: {k: (v.detach().cpu().to(self.dtype) if k != "step" else v.detach().cpu().clone())
                            for k, v in s.items()} for i, s in state_dict["state"].items()},
              "param_groups": self.opt.state_dict()["param_groups"]}
        self.opt.load_state_dict(sd)

    def set_lr(self, lr):
        for g in self.opt.param_groups:
            g["lr"] = lr

    def exp_avg(self, name):
        return self.opt.state[self.P[name]]["exp_avg"]

    def step(self, x, t, decisions=None, update=True):
        """returns (loss, accuracy, logits, {name: gradient}); the parameters and moments move when update"""
        x, t = x.to(self.dtype), t.to(self.dtype)
        logits = unet_forward(self.P, self.B, x, True, decisions)
        loss = F.binary_cross_entropy_with_logits(logits, t)
        self.opt.zero_grad()
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in self.P.items()}
        if update:
            self.opt.step()
        ld = logits.detach()
        acc = ((torch.sigmoid(ld) > 0.5).float() == (t > 0.5).float()).sum().item() / ld.numel()
        return float(loss.detach()), acc, ld, grads

    def state_dict(self):
        return {**{k: v.detach() for k, v in self.P.items()}, **self.B}
