"""The picture rules in numpy (checker only): what plt.imsave (matplotlib 3.10) writes for the reference's four calls
(models/model.py:505-518, models/segmentation_model.py:207), and floodgan's own rules where matplotlib has none.

  rgb_bytes      imsave(path, img, vmin=0, vmax=1) of a float32 H x W x 3 image: v = clip((x + 1) * 0.5, 0, 1) in
                 fp32 ("signed", utils.tensor_to_numpy) or clip(x, 0, 1) ("unit"); byte = trunc(v * 255) with the
                 product in fp32; alpha 255; NaN -> byte 0 (floodgan's rule)
  lut            the 256 x 4 byte table of "gray" / "gray_r": trunc(v * 255) in float64 of linspace(0, 1, 256) or
                 1 - linspace(0, 1, 256), alpha 255
  scalar_bytes   imsave(path, x, vmin=0, vmax=1, cmap=...): "unit" = lut[min(trunc(x * 256), 255)] with the product in
                 fp32, x < 0 -> entry 0, NaN -> RGBA 0 (floodgan's rule); "threshold" = x > 0.5 -> entry 255 else 0;
                 "logit" = sigmoid(x) > 0.5 (torch.sigmoid in fp32 on the CPU) -> entry 255 else 0
  LOGIT_BAND     |x| <= 2^-21: there an fp32 sigmoid may or may not round to exactly 0.5
"""
import numpy as np
import torch

LOGIT_BAND = 2.0 ** -21


def rgb_bytes(x, mode="signed"):
    """x: float32 [..., H, W, 3] (channels last) -> uint8 [..., H, W, 4]"""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore"):
        v = (x + np.float32(1)) * np.float32(0.5) if mode == "signed" else x
        assert v.dtype == np.float32
        v = np.clip(np.where(nan, np.float32(0), v), np.float32(0), np.float32(1))
        b = np.trunc(v * np.float32(255)).astype(np.uint8)
    b[nan] = 0
    out = np.empty(x.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = b
    out[..., 3] = 255
    return out


def lut(name):
    v = np.linspace(0, 1, 256)
    if name == "gray_r":
        v = 1 - v
    else:
        assert name == "gray", name
    t = np.empty((256, 4), dtype=np.uint8)
    t[:, :3] = np.trunc(v * 255).astype(np.uint8)[:, None]
    t[:, 3] = 255
    return t


def scalar_bytes(x, cmap="gray", kind="unit"):
    """x: float32 [..., H, W] -> uint8 [..., H, W, 4]"""
    x = np.asarray(x, dtype=np.float32)
    table = lut(cmap)
    if kind == "threshold":
        return table[np.where(x > np.float32(0.5), 255, 0)]
    if kind == "logit":
        flood = (torch.sigmoid(torch.from_numpy(np.ascontiguousarray(x))) > 0.5).numpy()
        return table[np.where(flood, 255, 0)]
    assert kind == "unit", kind
    nan = np.isnan(x)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(nan, np.float32(0), x) * np.float32(256)
        assert t.dtype == np.float32
        idx = np.clip(np.trunc(np.clip(t, np.float32(-1), np.float32(256))), 0, 255).astype(np.int64)
    out = table[idx]
    out[nan] = 0
    return out


def edge_values_rgb():
    """every bin edge 2k/255 - 1 of the signed RGB rule with its two fp32 neighbours, +-0, +-1, values beyond +-1 and
    a denormal (float32, 1-D, no NaN)"""
    k = np.arange(256, dtype=np.float64)
    e = (2 * k / 255 - 1).astype(np.float32)
    return np.concatenate([e, np.nextafter(e, np.float32(-9)), np.nextafter(e, np.float32(9)), _specials()])


def edge_values_scalar():
    """every bin edge k/256 of the colormap rule with its two fp32 neighbours, and the same specials"""
    e = (np.arange(257, dtype=np.float64) / 256).astype(np.float32)
    return np.concatenate([e, np.nextafter(e, np.float32(-9)), np.nextafter(e, np.float32(9)), _specials()])


def _specials():
    return np.array([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 3e38, -3e38, 1e-42, -1e-42, 0.5, -0.5,
                     0.49999997, 0.50000006], dtype=np.float32)
