"""Pin the segmentation training oracle (tests/seg_train_oracle.py) to golden numbers produced by the REAL
reference's SegmentationModel.train_model() (tests/golden/make_golden_segtrain.py): construction under
torch.manual_seed(5) (RNG order + initialise_weights), two epochs of two batches, (1, 3, 32, 32) then (2, 3, 32, 48),
at num_epochs=4 -- per-batch loss and accuracy, the learning rate of each epoch, and the parameter / BatchNorm buffer
checksums after each epoch.  Both sides run the same torch on the CPU: near bit-equality is expected."""
import os

import numpy as np
import pytest
import torch

import seg_train_oracle as SO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segtrain_32.npz")
NUM_EPOCHS, EPOCHS = 4, 2


def load_gold():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k.replace("__", "."): z[k] for k in z.files}


def synth_batches():
    """make_golden_segtrain.synth_batches: images ~ U[0, 1), masks (U > 0.6), one generator seeded 77"""
    g = torch.Generator().manual_seed(77)
    out = []
    for shape in ((1, 3, 32, 32), (2, 3, 32, 48)):
        x = torch.rand(shape, generator=g)
        t = (torch.rand((shape[0], 1) + shape[2:], generator=g) > 0.6).float()
        out.append((x, t))
    return out


def init_module():
    """the reference's construction: UNet() then initialise_weights under torch.manual_seed(5), on the CPU"""
    from floodgan.segmentation import UNet, initialise_weights
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5)
        return UNet().apply(initialise_weights)


def checksum(t):
    t = t.detach().double().flatten()
    idx = torch.linspace(0, t.numel() - 1, 16).long()
    return np.concatenate([[t.sum().item(), t.abs().sum().item()], t[:8].numpy(), t[idx].numpy()])


def check_state(gold, prefix, state, rtol):
    keys = {k[len(prefix) + 1:] for k in gold if k.startswith(prefix + "/")}
    assert keys == set(state), keys ^ set(state)
    for name, t in state.items():
        ref, mine = gold[f"{prefix}/{name}"], checksum(t)
        scale = max(abs(ref[1]), 1e-12)
        assert abs(mine[0] - ref[0]) / scale < rtol, (prefix, name, mine[0], ref[0])
        assert abs(mine[1] - ref[1]) / scale < rtol, (prefix, name, mine[1], ref[1])


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def test_init_rng_parity(gold):
    m = init_module()
    for name, t in m.state_dict().items():
        ref = gold[f"init/{name}"]
        n8 = min(8, t.numel())
        assert np.array_equal(t.double().flatten()[:n8].numpy(), ref[2:2 + n8]), name     # the same RNG stream


def test_lambda_rule(gold):
    for n in (1, 4, 100):
        mine = np.array([SO.lambda_rule(e, n) for e in range(n + 1)])
        assert np.array_equal(mine, gold[f"lambda_rule_{n}"]), n


def test_two_epochs_free_running(gold):
    torch.set_num_threads(8)
    st = SO.SegStepOracle(init_module(), torch.float32, num_epochs=NUM_EPOCHS)
    batches = synth_batches()
    for epoch in range(EPOCHS):
        lr = st.opt.param_groups[0]["lr"]
        assert abs(lr - gold["lr"][epoch]) <= 1e-12 * gold["lr"][epoch], (epoch, lr)
        for b, (x, t) in enumerate(batches):
            loss, acc, _, _ = st.step(x, t)
            ref = gold["losses"][epoch, b]
            assert abs(loss - ref) <= 1e-6 * abs(ref), (epoch, b, loss, ref)
            assert acc == gold["accuracies"][epoch, b], (epoch, b, acc)
        st.sched.step()
        check_state(gold, f"epoch{epoch + 1}", st.state_dict(), 1e-5)
