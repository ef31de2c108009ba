"""Pictures: generator outputs, attention masks and flood masks as PNG files, with the byte values of the
reference's plt.imsave calls (models/model.py:505-518, models/segmentation_model.py:207).

The reference's route is .cpu() -> numpy (utils.tensor_to_numpy) -> matplotlib.  Here the fp32 tensors are
converted and composed into an RGBA8 canvas on the device (csrc/render.hip: fg_render_rgb, fg_render_scalar), the
canvas crosses to the host in one copy of bytes -- a quarter of the fp32 data -- and floodgan.png encodes it.

  colormap_lut   the 256 RGBA entries matplotlib uses for "gray" / "gray_r"
  Canvas         a device uint8 [H, W, 4] picture with a pinned host mirror: .rgb / .scalar / .host / .save
  save_image     one tensor -> one PNG: the four plt.imsave calls of the reference
  sheet_layout   where the panels of an image sheet sit (native resolution, white 8-px gutters, no outer margin)
  save_sheet     rows x columns of panels -> one PNG with a `floodgan:panels` tEXt chunk naming them

Sheets carry no titles (there is no font rendering here) and are not claimed to match matplotlib's figures; the
panels inside them are the imsave bytes.
"""
import json

import numpy as np
import torch

from . import ops
from .plans import Buf
from .png import write_png

PANELS_KEY = "floodgan:panels"
# save_image's kinds: (colormap, scalar kind) or None for RGB
_IMAGE_KINDS = {"rgb": None, "attention": ("gray_r", "unit"), "mask_logits": ("gray", "logit"),
                "mask_true": ("gray", "threshold")}


def colormap_lut(name):
    """matplotlib's byte table of the linear colormaps "gray" and "gray_r" as uint8 [256, 4]: entry i is
    trunc(v_i * 255) in float64 with v = linspace(0, 1, 256) (gray) or 1 - linspace(0, 1, 256) (gray_r), alpha 255.
    Not i / 255 - i: the truncation of i / 255 * 255 falls one short at some entries."""
    v = np.linspace(0, 1, 256)
    if name == "gray_r":
        v = 1 - v
    elif name != "gray":
        raise NotImplementedError(f"colormap {name!r}: floodgan renders 'gray' and 'gray_r'")
    lut = np.empty((256, 4), dtype=np.uint8)
    lut[:, :3] = (v * 255).astype(np.uint8)[:, None]
    lut[:, 3] = 255
    return lut


_DEVICE_LUTS = {}


def device_lut(name, device):
    """colormap_lut(name) on `device`, cached per device"""
    key = (name, str(torch.device(device)))
    if key not in _DEVICE_LUTS:
        _DEVICE_LUTS[key] = torch.from_numpy(colormap_lut(name)).to(device)
    return _DEVICE_LUTS[key]


class Canvas:
    """An RGBA8 picture on the device (uint8 [height, width, 4]; rows pitched to 16 bytes so that panels at
    columns that are multiples of 4 take the kernels' 16-byte stores) with a pinned host mirror."""

    def __init__(self, height, width, device="cuda", fill=(255, 255, 255, 255)):
        if height < 1 or width < 1:
            raise ValueError(f"Canvas: {height} x {width}")
        pitch = (width + 3) // 4 * 4
        self._dev = torch.empty((height, pitch, 4), dtype=torch.uint8, device=device)
        self._dev[:] = torch.tensor(fill, dtype=torch.uint8, device=device)       # the gutters: plain torch
        self._host = torch.empty((height, pitch, 4), dtype=torch.uint8, pin_memory=True)
        self.height, self.width = height, width
        self.pixels = self._dev[:, :width]

    def rgb(self, t, row=0, col=0, unit=False, step_rows=0, step_cols=0):
        ops.render_rgb(t, self.pixels, row, col, unit, step_rows, step_cols)
        return self

    def scalar(self, t, row=0, col=0, cmap="gray", kind="unit", step_rows=0, step_cols=0):
        dev = t.t.device if isinstance(t, Buf) else t.device
        ops.render_scalar(t, device_lut(cmap, dev), self.pixels, row, col, kind, step_rows, step_cols)
        return self

    def host(self):
        """the picture as a uint8 [height, width, 4] numpy view of the pinned mirror: one asynchronous copy on the
        current stream, then a wait on its event (valid until the next .host())"""
        self._host.copy_(self._dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        return self._host.numpy()[:, :self.width]

    def save(self, path, text=None):
        write_png(path, self.host(), text=text)
        return path


def save_image(path, tensor, kind="rgb", unit=False):
    """The single-image plt.imsave calls of the reference on the device: kind "rgb" (imsave(img, vmin=0, vmax=1)
    of tensor_to_numpy's (x + 1) / 2, or of clip(x, 0, 1) with unit=True), "attention" (cmap="gray_r" over 0..1,
    the mask as it is), "mask_logits" (cmap="gray" of sigmoid(x) > 0.5) or "mask_true" (cmap="gray" of x > 0.5).
    The first image of a batch is written."""
    if kind not in _IMAGE_KINDS:
        raise NotImplementedError(f"save_image: kind must be one of {sorted(_IMAGE_KINDS)} (got {kind!r})")
    t = tensor.interior().permute(0, 3, 1, 2) if isinstance(tensor, Buf) else tensor
    if kind == "rgb":
        t = t[:1] if t.dim() == 4 else t
    else:
        t = t[:1] if t.dim() >= 3 else t
    h, w = t.shape[-2], t.shape[-1]
    cv = Canvas(h, w, t.device)
    if kind == "rgb":
        cv.rgb(t, unit=unit)
    else:
        cv.scalar(t, cmap=_IMAGE_KINDS[kind][0], kind=_IMAGE_KINDS[kind][1])
    return cv.save(path)


def sheet_layout(n_rows, n_cols, h, w, gutter=8):
    """(height, width, offsets) of a sheet of n_rows x n_cols panels of h x w pixels at native resolution: a gutter
    between neighbours, no outer margin; offsets[r][c] = (row, col) of panel (r, c)'s top-left pixel."""
    if min(n_rows, n_cols, h, w) < 1 or gutter < 0:
        raise ValueError(f"sheet_layout: {n_rows} x {n_cols} panels of {h} x {w}, gutter {gutter}")
    offsets = [[(r * (h + gutter), c * (w + gutter)) for c in range(n_cols)] for r in range(n_rows)]
    return n_rows * h + (n_rows - 1) * gutter, n_cols * w + (n_cols - 1) * gutter, offsets


def _rows_of(t, scalar):
    """(rows, h, w) of a column piece: a tensor batch or an NHWC Buf"""
    if isinstance(t, Buf):
        return t.n, t.h, t.w
    if t.dim() < (3 if scalar else 4):
        raise ValueError(f"save_sheet: a column piece is a batch (got shape {tuple(t.shape)})")
    return t.shape[0], t.shape[-2], t.shape[-1]


def save_sheet(path, columns, row_names, gutter=8):
    """One sheet: columns = [(title, kind, batch)] with kind as save_image's, or "rgb_unit"; batch holds the sheet's
    rows in order: one tensor ([R, C, H, W]; [R, H, W] or [R, 1, H, W] for the scalar kinds; or an NHWC Buf), placed
    with one launch (step_rows), or a list of such pieces when the rows come from several batches.  Returns the
    panels dict that the file carries as JSON in its `floodgan:panels` tEXt chunk."""
    n_rows = len(row_names)
    cols = [(title, kind, list(b) if isinstance(b, (list, tuple)) else [b]) for title, kind, b in columns]
    _, h, w = _rows_of(cols[0][2][0], cols[0][1] not in ("rgb", "rgb_unit"))
    height, width, offsets = sheet_layout(n_rows, len(cols), h, w, gutter)
    first = cols[0][2][0]
    cv = Canvas(height, width, first.t.device if isinstance(first, Buf) else first.device)
    for c, (_, kind, pieces) in enumerate(cols):
        scalar = kind not in ("rgb", "rgb_unit")
        if scalar and kind not in _IMAGE_KINDS:
            raise NotImplementedError(f"save_sheet: unknown panel kind {kind!r}")
        r = 0
        for t in pieces:
            k, th, tw = _rows_of(t, scalar)
            if (th, tw) != (h, w) or r + k > n_rows:
                raise ValueError(f"save_sheet: column {c}: {k} panels of {th} x {tw} at row {r} of a sheet of "
                                 f"{n_rows} rows of {h} x {w}")
            row, col = offsets[r][c]
            if scalar:
                cv.scalar(t, row, col, cmap=_IMAGE_KINDS[kind][0], kind=_IMAGE_KINDS[kind][1], step_rows=h + gutter)
            else:
                cv.rgb(t, row, col, unit=kind == "rgb_unit", step_rows=h + gutter)
            r += k
        if r != n_rows:
            raise ValueError(f"save_sheet: column {c} holds {r} panels for {n_rows} rows")
    panels = {"columns": [title for title, _, _ in cols], "rows": [str(r) for r in row_names],
              "panel": [h, w], "gutter": gutter}
    cv.save(path, text={PANELS_KEY: json.dumps(panels)})
    return panels
