"""Writes tests/golden/render_imsave.npz: small fp32 images and the RGBA bytes matplotlib's plt.imsave produced for
them (read back from the PNG), the three calls of the reference's pictures --

    plt.imsave(path, img, vmin=0, vmax=1)                        models/model.py:505-513 (img = tensor_to_numpy(...))
    plt.imsave(path, mask, vmin=0, vmax=1, cmap="gray_r")        models/model.py:518
    plt.imsave(path, mask01, vmin=0, vmax=1, cmap="gray")        models/segmentation_model.py:207

-- and the 256 x 4 byte tables of the two colormaps.  The inputs hold every bin edge of the quantisation with its two
fp32 neighbours, +-0, +-1, values beyond +-1 and a denormal, and no NaN (tests/render_oracle.py: edge_values_*).
Needs matplotlib (Agg) and PIL; run from the repository root:  python tests/golden/make_golden_render.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
from PIL import Image  # noqa: E402

import render_oracle as RO  # noqa: E402


def imsave_bytes(img, **kw):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "a.png")
        plt.imsave(path, img, vmin=0, vmax=1, **kw)
        with Image.open(path) as im:
            assert im.mode == "RGBA", im.mode
            return np.asarray(im, dtype=np.uint8).copy()


def fill(values, shape, rng, lo, hi):
    """`values` scattered over an array of `shape`, the rest uniform in [lo, hi)"""
    n = int(np.prod(shape))
    assert values.size <= n, (values.size, n)
    flat = rng.uniform(lo, hi, n).astype(np.float32)
    flat[rng.permutation(n)[:values.size]] = values
    return flat.reshape(shape)


def signed_to_imsave(x):
    """utils.tensor_to_numpy (models/utils.py:12-17) on an H x W x 3 float32 array"""
    return np.clip((x + 1) * 0.5, 0, 1)


def main():
    rng = np.random.default_rng(47)
    rgb_in = fill(RO.edge_values_rgb(), (24, 40, 3), rng, -1.2, 1.2)
    gray_r_in = fill(RO.edge_values_scalar(), (48, 80), rng, -0.2, 1.2)
    gray_in = (rng.uniform(0, 1, (16, 20)) > 0.5).astype(np.float32)
    pre = signed_to_imsave(rgb_in)
    assert pre.dtype == np.float32 and not np.isnan(rgb_in).any() and not np.isnan(gray_r_in).any()
    out = dict(rgb_in=rgb_in, rgb_out=imsave_bytes(pre),
               gray_r_in=gray_r_in, gray_r_out=imsave_bytes(gray_r_in, cmap="gray_r"),
               gray_in=gray_in, gray_out=imsave_bytes(gray_in, cmap="gray"),
               lut_gray=matplotlib.colormaps["gray"](np.arange(256), bytes=True),
               lut_gray_r=matplotlib.colormaps["gray_r"](np.arange(256), bytes=True),
               matplotlib_version=np.array(matplotlib.__version__))
    path = os.path.join(HERE, "render_imsave.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: getattr(v, "shape", None) for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
