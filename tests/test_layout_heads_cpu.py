"""The reference-side half of what tests/test_gpu_bnorm.py and tests/test_gpu_layout_heads.py claim to see, on the
CPU: the chunk arithmetic their case comments state, and that the edges they aim at move the fp64 reference by many
times the kernel bound (so a kernel that mishandles them cannot pass)."""
import torch
import torch.nn.functional as F

KTOL = 1e-5
MAX_PARTIALS = 1024


def chunks_of(groups, hw):
    """choose_chunks of csrc/bnorm.hip and the pixels per chunk the statistics kernels derive from it"""
    c = max(1, min(MAX_PARTIALS // groups, hw // 16))
    return c, -(-hw // c)


def test_chunk_arithmetic_of_the_batchnorm_cases():
    assert chunks_of(1, 17 * 17) == (18, 17) and 17 * 17 == 289                 # chunk 17 starts at 289: empty
    assert chunks_of(3, 7 * 9) == (3, 21)
    c, per = chunks_of(2, 33 * 31)
    assert (c, per) == (63, 17) and 60 * per < 1023 <= 61 * per                  # chunks 61, 62 start past the end
    c, per = chunks_of(1, 128 * 130)
    assert (c, per) == (MAX_PARTIALS, 17) and 978 * per < 16640 <= 979 * per     # the chunks from 979 on are empty
    assert 4 * 128 * 130 * (64 // 4) == 1064960 > 4096 * 256                      # both apply kernels iterate twice
    assert chunks_of(8, 25) == (1, 25) and chunks_of(1, 15) == (1, 15) and chunks_of(2, 16) == (1, 16)
    c, per = chunks_of(1, 9 * 11)
    assert (c, per) == (6, 17) and 99 - 5 * per == 14
    # the earlier cases: the chunks divide the pixels, no partial or empty chunk
    for groups, hw in ((1, 64), (2, 192), (1, 4096), (2, 4096)):
        c, per = chunks_of(groups, hw)
        assert c * per == hw


def test_a_dropped_chunk_tail_moves_batchnorm_far_beyond_the_bound():
    """per = HW / chunks rounded down leaves pixel 288 of 289 out of the statistics: the fp64 output then moves by
    3.6e-3 of its maximum, 360 times the kernel bound (asserted: at least twenty times)"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, 17, 17, generator=g, dtype=torch.float64) * 1.7 + 0.6
    full = F.batch_norm(x, None, None, training=True, eps=1e-5)
    flat = x.flatten(2)[..., :288]
    mean, var = flat.mean((0, 2)), flat.var((0, 2), unbiased=False)
    short = (x - mean[None, :, None, None]) / torch.sqrt(var + 1e-5)[None, :, None, None]
    moved = float((short - full).abs().max() / full.abs().max())
    assert moved > 20 * KTOL, moved


def test_softmax_without_max_subtraction_overflows_where_the_tail_test_looks():
    """ten equal logits at 100: exp overflows in fp32 and the plain quotient is inf / inf = NaN, the max-subtracted one
    float32(0.1) (at -100 too); a spread of +-80 alone would not show it (exp(80) is finite in fp32)"""
    al = torch.full((10,), 100.0, dtype=torch.float32)
    assert bool(torch.isnan(torch.exp(al) / torch.exp(al).sum()).all())
    for v in (100.0, -100.0):
        al = torch.full((10,), v, dtype=torch.float32)
        assert bool((torch.softmax(al, 0) == torch.tensor(0.1, dtype=torch.float32)).all())
    assert bool(torch.isfinite(torch.exp(torch.tensor(80.0, dtype=torch.float32))))


def test_reflect_adjoint_has_three_preimages_at_the_smallest_size():
    """at (fold + 1) x (fold + 2) an interior index is the image of three padded ones (itself, the lower and the
    upper reflection) along w, and along h too from fold 2 on: the adjoint sums up to 9 terms there (6 at fold 1),
    against 4 at most at 13 x 17"""
    for fold, h, w, most in ((3, 4, 5, 9), (1, 2, 3, 6), (3, 13, 17, 4)):
        x = torch.zeros(1, 1, h, w, dtype=torch.float64, requires_grad=True)
        (count,) = torch.autograd.grad(F.pad(x, (fold,) * 4, mode="reflect").sum(), x)
        assert int(count.max()) == most


def test_tanh_derivative_vanishes_in_fp32_from_20_on():
    t = torch.tanh(torch.tensor([20.0, -20.0, 40.0], dtype=torch.float32))
    assert bool((1 - t * t == 0).all())
    assert float((1 - torch.tanh(torch.tensor(20.0, dtype=torch.float64)) ** 2)) < 1e-15
