"""numpy fp64 oracle of the scene mosaic (floodgan.scene, csrc/mosaic.hip): the window grid, the blending weight and
the blend, restated from their definitions and independent of the package.

  starts(L, tile, overlap)   the sorted unique values of min(i S, L - tile), i = 0 .. ceil((L - tile) / S), S = tile -
                             overlap
  weight(tile, overlap)      w(u) = min(u + 1, tile - u, max(overlap, 1)), u = 0 .. tile - 1
  coverage(L, tile, overlap) how many windows cover each coordinate of an axis, and the axis' weight sums
  blend(windows, ...)        sum_k(w_k v_k) / sum_k(w_k) in fp64, window k = iy len(xs) + ix at (ys[iy], xs[ix])
"""
import math

import numpy as np


def starts(L, tile, overlap):
    S = tile - overlap
    return sorted({min(i * S, L - tile) for i in range(math.ceil((L - tile) / S) + 1)})


def weight(tile, overlap):
    return np.array([min(u + 1, tile - u, max(overlap, 1)) for u in range(tile)], dtype=np.int64)


def coverage(L, tile, overlap):
    """(number of windows, weight sum) per coordinate of an axis of length L"""
    count, wsum = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    for s in starts(L, tile, overlap):
        count[s:s + tile] += 1
        wsum[s:s + tile] += weight(tile, overlap)
    return count, wsum


def blend(windows, H, W, tile, overlap):
    """windows [K, c, tile, tile] (any float dtype) -> the blended [c, H, W] image in fp64"""
    ys, xs = starts(H, tile, overlap), starts(W, tile, overlap)
    windows = np.asarray(windows, dtype=np.float64)
    assert windows.shape[0] == len(ys) * len(xs) and windows.shape[2:] == (tile, tile), windows.shape
    w1 = weight(tile, overlap).astype(np.float64)
    w2 = w1[:, None] * w1[None, :]
    num = np.zeros((windows.shape[1], H, W), dtype=np.float64)
    den = np.zeros((H, W), dtype=np.float64)
    for k in range(windows.shape[0]):
        y0, x0 = ys[k // len(xs)], xs[k % len(xs)]
        num[:, y0:y0 + tile, x0:x0 + tile] += w2 * windows[k]
        den[y0:y0 + tile, x0:x0 + tile] += w2
    assert den.min() >= 1
    return num / den
