"""The scene mosaic's host arithmetic (floodgan.scene.window_grid, window_weight) and its numpy oracle
(tests/scene_oracle.py): exact integers, no device."""
import numpy as np
import pytest

import scene_oracle as SO
from tiff_util import write_tiff

# (L, tile, S = tile - overlap) -> the window starts along an axis of length L
AXES = {(40, 16, 8): [0, 8, 16, 24],
        (52, 16, 12): [0, 12, 24, 36],
        (16, 16, 8): [0],
        (17, 16, 8): [0, 1],
        (88, 32, 24): [0, 24, 48, 56],
        (72, 32, 16): [0, 16, 32, 40],
        (33, 16, 16): [0, 16, 17],
        (100, 32, 32): [0, 32, 64, 68]}


@pytest.mark.parametrize("L,tile,S", list(AXES))
def test_window_grid_exact_starts(L, tile, S):
    from floodgan.scene import window_grid
    want = AXES[(L, tile, S)]
    overlap = tile - S
    ys, xs = window_grid(L, L, tile, overlap)
    assert ys == want and xs == want and all(isinstance(v, int) for v in ys)
    # the axes are independent: as the columns of a scene one window high, and as the rows of one 100 wide
    assert window_grid(tile, L, tile, overlap) == ([0], want)
    assert window_grid(L, 100, tile, overlap) == (want, SO.starts(100, tile, overlap))
    assert SO.starts(L, tile, overlap) == want


@pytest.mark.parametrize("L,tile,S", list(AXES))
def test_every_coordinate_is_covered_at_most_three_times(L, tile, S):
    from floodgan.scene import window_grid, window_weight
    overlap = tile - S
    _, xs = window_grid(tile, L, tile, overlap)
    w = window_weight(tile, overlap)
    assert np.array_equal(w, SO.weight(tile, overlap)) and w.min() == 1 and w.max() == max(overlap, 1)
    assert np.array_equal(w, w[::-1])
    count, wsum = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    for s in xs:
        assert 0 <= s and s + tile <= L                       # every window lies inside the scene
        count[s:s + tile] += 1
        wsum[s:s + tile] += w
    assert count.min() >= 1 and count.max() <= 3 and wsum.min() >= 1
    ocount, owsum = SO.coverage(L, tile, overlap)
    assert np.array_equal(count, ocount) and np.array_equal(wsum, owsum)
    if (L, tile, S) == (72, 32, 16):
        assert count.max() == 3                               # the triple coverage
    # the largest admissible overlap keeps a pixel's weight sum (<= 9 windows) exact in fp32
    assert 9 * 1024 * 1024 < 2 ** 24


def test_window_grid_refusals_name_the_value():
    from floodgan.scene import Mosaic, window_grid
    with pytest.raises(ValueError, match="tile 48"):
        window_grid(40, 64, 48, 8)
    with pytest.raises(ValueError, match="tile 48"):
        window_grid(64, 40, 48, 8)
    with pytest.raises(ValueError, match="overlap -1"):
        window_grid(64, 64, 16, -1)
    with pytest.raises(ValueError, match="overlap 9"):
        window_grid(64, 64, 16, 9)
    with pytest.raises(ValueError, match="overlap 1025"):
        window_grid(8192, 8192, 4096, 1025)
    assert window_grid(8192, 8192, 4096, 1024) == ([0, 3072, 4096], [0, 3072, 4096])
    assert window_grid(64, 64, 16, 8)[0] == [0, 8, 16, 24, 32, 40, 48]
    with pytest.raises(ValueError, match="c must be 1 or 3"):
        Mosaic(64, 64, 2, 16, 8, "cpu")


def test_oracle_constant_windows_blend_to_the_constant():
    for (H, W, tile, overlap) in [(41, 53, 16, 8), (72, 40, 32, 16), (33, 48, 16, 0)]:
        k = len(SO.starts(H, tile, overlap)) * len(SO.starts(W, tile, overlap))
        out = SO.blend(np.full((k, 3, tile, tile), 0.37), H, W, tile, overlap)
        assert out.shape == (3, H, W) and np.abs(out - 0.37).max() < 1e-15


def test_oracle_one_window_returns_it():
    rng = np.random.default_rng(3)
    win = rng.uniform(-1, 1, (1, 3, 16, 16))
    assert np.abs(SO.blend(win, 16, 16, 16, 8) - win[0]).max() < 1e-15


def test_oracle_overlap_is_the_weighted_mean_of_two_windows():
    """two windows over a row of 24 pixels (tile 16, overlap 8): inside the overlap the weights ramp 8..1 against 1..8"""
    a, b = np.full((1, 16, 16), 1.0), np.full((1, 16, 16), -1.0)
    out = SO.blend(np.stack([a, b]), 16, 24, 16, 8)
    assert SO.starts(24, 16, 8) == [0, 8]
    for x in range(24):
        wa = min(x + 1, 16 - x, 8) if x < 16 else 0
        wb = min(x - 8 + 1, 16 - (x - 8), 8) if x >= 8 else 0
        assert abs(out[0, 5, x] - (wa - wb) / (wa + wb)) < 1e-15


def test_new_names_are_exported():
    import floodgan
    from floodgan import data, model, scene
    for name in ("Mosaic", "predict_scene", "window_grid"):
        assert name in floodgan.__all__ and getattr(floodgan, name) is getattr(scene, name)
    assert callable(data.load_scene) and callable(model.Model.predict_scene)
    from floodgan import _lib as L
    assert {"fg_mosaic_accumulate", "fg_mosaic_finalize"} <= set(L.SIGNATURES)


def test_load_scene_refuses_a_channel_count_it_cannot_map(tmp_path):
    from floodgan.data import load_scene
    path = str(tmp_path / "scene.tif")
    write_tiff(path, np.random.default_rng(1).random((12, 20, 5)).astype(np.float32))
    with pytest.raises(ValueError, match="5 channels.*9-channel.*4 channels"):
        load_scene(path, "dem", "cpu")
    with pytest.raises(ValueError, match="5 channels.*9-channel.*9 channels"):
        load_scene(path, "all", "cpu")
