"""Whole scenes: windowed inference with overlap blending.

The generators train on tiles (512^2 quadrants, 256^2 resizes) and their executors take tile-shaped inputs only; a
scene a user wants a flood prediction for is larger and of any size.  The reference's only answer is the quadrant
crop: four pictures with InstanceNorm seams between them.  Here a scene is cut into overlapping training-size
windows, the windows run through the generator in batches, and their outputs are blended back into one image on the
device (csrc/mosaic.hip: fg_mosaic_accumulate, fg_mosaic_finalize).  Not in the reference.

  window_grid    the window starts of an H x W scene: exact integer arithmetic (the CPU tests cover it)
  window_weight  the integer blending weight of a window-local coordinate
  Mosaic         the fp32 accumulation planes and the device grid: .windows / .add / .result
  predict_scene  scene -> generator output, and with a segmentation U-Net its flood logits and flood fraction; with
                 min_region / min_hole also the sieved flood mask and its regions (floodgan.regions), with polygons
                 their outlines (floodgan.outline)

Grid.  Along an axis of length L, with S = tile - overlap, the starts are the sorted unique values of
min(i S, L - tile), i = 0 .. ceil((L - tile) / S): every window lies inside the scene, the last one shifted inward
rather than padded.  Window k = iy len(xs) + ix.  With overlap <= tile // 2 at most three windows cover a coordinate
along one axis, nine a pixel.
Weight.  w(u) = min(u + 1, tile - u, max(overlap, 1)) at window-local coordinate u: a ramp of `overlap` pixels at each
edge, flat inside.  A pixel's weight in a window is w(y - y0) w(x - x0); the blended value is sum_k(w_k v_k) /
sum_k(w_k) over the covering windows.  overlap <= 1024 keeps every weight (<= 2^20) and weight sum (< 2^24) exact in
fp32.  The sum runs in ascending k with the product and the add as separate fp32 operations, so the result does not
depend on how the windows are split into batches.

Out of scope: mosaics of the attention masks (last_attention_mask after predict_scene is the last batch's),
reflect-padding of scenes smaller than a window (tile > H or W is refused), GeoTIFF output, and any change to
Model.plot_image.
"""
import os

import numpy as np
import torch

from . import ops
from ._lib import FG_MOSAIC_MAX_OVERLAP, require_device
from .plans import Buf

MAX_OVERLAP = FG_MOSAIC_MAX_OVERLAP


def _starts(length, tile, overlap):
    step = tile - overlap
    last = length - tile
    return sorted({min(i * step, last) for i in range(-(-last // step) + 1)})


def window_grid(H, W, tile, overlap):
    """(ys, xs): the window starts along the rows and the columns of an H x W scene (module docstring).  Raises
    ValueError for tile > H or W, overlap < 0, overlap > tile // 2 and overlap > 1024."""
    H, W, tile, overlap = int(H), int(W), int(tile), int(overlap)
    if tile < 1:
        raise ValueError(f"window_grid: tile {tile} must be positive")
    if tile > H or tile > W:
        raise ValueError(f"window_grid: tile {tile} is larger than the {H} x {W} scene (scenes smaller than a window "
                         "are not padded)")
    if overlap < 0:
        raise ValueError(f"window_grid: overlap {overlap} is negative")
    if overlap > tile // 2:
        raise ValueError(f"window_grid: overlap {overlap} is more than half the tile ({tile} // 2 = {tile // 2}): "
                         "more than three windows would cover a coordinate")
    if overlap > MAX_OVERLAP:
        raise ValueError(f"window_grid: overlap {overlap} is above {MAX_OVERLAP}, the bound that keeps the blending "
                         "weights exact in fp32")
    return _starts(H, tile, overlap), _starts(W, tile, overlap)


def window_weight(tile, overlap):
    """w(u) for u = 0 .. tile - 1 as an int64 numpy array"""
    u = np.arange(tile, dtype=np.int64)
    return np.minimum(np.minimum(u + 1, tile - u), max(int(overlap), 1))


class Mosaic:
    """The blend of one H x W scene with c (1 or 3) channels: fp32 accumulation planes [c, H, W] and the window grid,
    both on `device`.  Windows are added in batches of consecutive indices, in ascending order, each once:
    add(windows, k0) takes windows k0 .. k0 + n - 1 as an [n, >= c, tile, tile] tensor of any strides or as an NHWC
    Buf (its channels 0 .. c - 1), result() the blended [1, c, H, W] image once every window is in.  The result is
    bit-identical for every split into batches."""

    def __init__(self, H, W, c, tile, overlap, device="cuda"):
        if c not in (1, 3):
            raise ValueError(f"Mosaic: c must be 1 or 3 (got {c})")
        self.ys, self.xs = window_grid(H, W, tile, overlap)
        self.H, self.W, self.c, self.tile, self.overlap = int(H), int(W), c, int(tile), int(overlap)
        self.device = torch.device(device)
        self._host = tuple(np.asarray(s, dtype=np.int32) for s in (self.ys, self.xs))
        self._dev = tuple(torch.from_numpy(s).to(self.device) for s in self._host)
        self.grid_struct = ops.mosaic_grid_struct(*self._dev, *self._host, self.tile, self.overlap)
        self.planes = torch.zeros((c, self.H, self.W), dtype=torch.float32, device=self.device)
        self.added = 0

    @property
    def grid(self):
        return self.ys, self.xs

    @property
    def count(self):
        return len(self.ys) * len(self.xs)

    def corner(self, k):
        """(y0, x0) of window k"""
        return self.ys[k // len(self.xs)], self.xs[k % len(self.xs)]

    def batches(self, batch):
        """(k0, n) of the batches of at most `batch` windows, in order; the last may be smaller"""
        if batch < 1:
            raise ValueError(f"Mosaic: batch {batch} must be positive")
        return [(k0, min(batch, self.count - k0)) for k0 in range(0, self.count, batch)]

    def windows(self, x, k0, n):
        """windows k0 .. k0 + n - 1 of a device scene [1, C, H, W] as one [n, C, tile, tile] batch (plain torch)"""
        if x.dim() != 4 or x.shape[0] != 1 or tuple(x.shape[2:]) != (self.H, self.W):
            raise ValueError(f"Mosaic.windows: a [1, C, {self.H}, {self.W}] scene (got {tuple(x.shape)})")
        if k0 < 0 or n < 1 or k0 + n > self.count:
            raise ValueError(f"Mosaic.windows: windows {k0} .. {k0 + n - 1} of {self.count}")
        t = self.tile
        return torch.stack([x[0, :, y0:y0 + t, x0:x0 + t] for y0, x0 in map(self.corner, range(k0, k0 + n))])

    def add(self, windows, k0):
        n = windows.n if isinstance(windows, Buf) else windows.shape[0]
        if k0 != self.added or k0 + n > self.count:
            raise ValueError(f"Mosaic.add: windows {k0} .. {k0 + n - 1} after {self.added} of {self.count}: batches "
                             "arrive in ascending order, each window once")
        ops.mosaic_accumulate(windows, k0, self.grid_struct, self.planes)
        self.added += n
        return self

    def reset(self):
        """zero planes, no window added: ready for the next scene of the same geometry"""
        self.planes.zero_()
        self.added = 0
        return self

    def result(self):
        if self.added != self.count:
            raise RuntimeError(f"Mosaic.result: {self.added} of {self.count} windows added")
        out = torch.empty((1, self.c, self.H, self.W), dtype=torch.float32, device=self.device)
        ops.mosaic_finalize(self.planes, self.grid_struct, out)
        return out


def _unet(seg_model, batch_stats):
    """a drop-in UNet, a SegmentationModel or a checkpoint path -> the UNet, resolved as FloodMaskLoss resolves it"""
    from .segmentation import FloodMaskLoss
    return FloodMaskLoss(seg_model, batch_stats).seg


def _flood_logits(unet, images, batch_stats):
    """the frozen U-Net's logits Buf of an [n, 3, h, w] batch in [-1, 1]: fg_unit_image into the U-Net's input, then
    unet_logits on the running statistics (or each batch's own), nothing written to the module"""
    from .segmentation import unet_logits, unit_image
    _, X0 = unit_image(images, buf=True, nchw=False)
    return unet_logits(dict(unet.named_parameters()), dict(unet.named_buffers()), X0, batch_stats,
                       update_running=False)


def predict_scene(generator, x, tile=512, overlap=64, batch=8, seg_model=None, batch_stats=False, min_region=None,
                  min_hole=None, connectivity=8, elevation=None, pixel_area=1.0, polygons=False, drainage=False,
                  flat_rounds=0):
    """A device scene x [1, C, H, W] in [-1, 1] through `generator` in windows of tile x tile pixels, `batch` at a
    time (the last batch may be smaller), blended by Mosaic.  Runs under torch.no_grad() with torch.manual_seed(47)
    before each generator call, as the package's picture paths do; the generator runs in the mode it is in.
    Returns {"output": [1, 3, H, W] fp32, "grid": (ys, xs)} and, with seg_model (a drop-in UNet, a SegmentationModel
    or a checkpoint path, as FloodMaskLoss takes them), "flood_logits": [1, 1, H, W] -- the frozen U-Net's logits of
    the windows of the blended output (through fg_unit_image), blended by the same mosaic -- and "flood_fraction":
    the share of pixels whose blended logit is a flood by the decision of fg_mask_confusion, counted on the device.
    batch_stats=False: the U-Net's BatchNorm on its running statistics; True: on each batch's own; its parameters and
    buffers are never written.  tile must then be a multiple of 16 (ValueError before any launch).
    A scene that is exactly one window returns the generator's output as it is, without a blend.  tile=None: one
    window over the whole scene, whatever its shape (the generator's own size check applies).
    min_region / min_hole (either given, with seg_model; ValueError without): the flood-extent product of the blended
    logits (floodgan.regions.flood_regions with the minima -- None is "off" -- and `connectivity`): the result gains
    "flood_mask" (fp32 [1, 1, H, W] of 0 / 1, sieved), "regions" (flood_regions' dict without its mask) and
    "flood_fraction_sieved"; "flood_logits" and "flood_fraction" are what they are without the minima.
    elevation (fp32 [H, W] or [1, 1, H, W] on the scene's device, with seg_model; ValueError without, or on another
    shape or device, before any launch): the depth product of the flood mask (floodgan.depth.flood_depth with the
    regions and `pixel_area`) -- of the sieved mask when minima are given, else of the plain decision, which the
    result then also carries as "flood_mask" and "regions" (flood_regions with the minima off).  The result gains
    "flood_depth" (fp32 [1, 1, H, W]) and "depth" (flood_depth's dict without its plane).
    polygons=True (with seg_model; ValueError without, before any launch): the outlines of the regions
    (floodgan.outline.region_outlines of the regions' labels at `connectivity`), with "flood_mask" and "regions" as
    `elevation` gives them (the minima off unless given).  The result gains "outlines".
    drainage=True (with elevation; ValueError without, before any launch; seg_model is not needed, and without it the
    elevation gives no depth): the drainage of the elevation (floodgan.flow.flow_accumulation with `flat_rounds`).
    The result gains "flow" (flow_accumulation's dict) and, when the regions are computed, their table gains
    "max_accumulation" and "pit_pixels" (floodgan.flow.flow_region_table), which "flow" also carries as "table".
    Out of scope: attention-mask mosaics, reflect-padding of scenes smaller than a window, GeoTIFF output."""
    if drainage:
        from .flow import check_flat_rounds
        if elevation is None:
            raise ValueError("predict_scene: drainage=True routes flow over the scene's elevation and needs elevation")
        flat_rounds = check_flat_rounds(flat_rounds)
    if elevation is not None and seg_model is None and not drainage:
        raise ValueError("predict_scene: elevation gives the depth of the flood mask and needs seg_model")
    if polygons and seg_model is None:
        raise ValueError("predict_scene: polygons=True outlines the regions of the flood mask and needs seg_model")
    if polygons and connectivity not in (4, 8):
        raise ValueError(f"predict_scene: connectivity {connectivity!r} must be 4 or 8")
    require_device(x, "scene")
    if x.dim() != 4 or x.shape[0] != 1:
        raise ValueError(f"predict_scene: a [1, C, H, W] scene (got {tuple(x.shape)})")
    H, W = int(x.shape[2]), int(x.shape[3])
    if elevation is not None:
        if connectivity not in (4, 8):
            raise ValueError(f"predict_scene: connectivity {connectivity!r} must be 4 or 8")
        if not (torch.is_tensor(elevation) and elevation.dtype == torch.float32
                and tuple(elevation.shape) in ((H, W), (1, 1, H, W)) and elevation.device == x.device):
            raise ValueError(f"predict_scene: the elevation must be a float32 [{H}, {W}] or [1, 1, {H}, {W}] tensor on "
                             f"{x.device} (got {getattr(elevation, 'dtype', type(elevation))} "
                             f"{tuple(getattr(elevation, 'shape', ()))} on {getattr(elevation, 'device', 'the host')})")
    if batch < 1:
        raise ValueError(f"predict_scene: batch {batch} must be positive")
    whole = tile is None
    ys, xs = ([0], [0]) if whole else window_grid(H, W, tile, overlap)
    unet = None
    sieve = min_region is not None or min_hole is not None
    min_region, min_hole = 1 if min_region is None else int(min_region), 0 if min_hole is None else int(min_hole)
    if sieve:
        if seg_model is None:
            raise ValueError("predict_scene: min_region / min_hole sieve the flood mask and need seg_model")
        if min_region < 0 or min_hole < 0 or connectivity not in (4, 8):
            raise ValueError(f"predict_scene: min_region {min_region} and min_hole {min_hole} must not be negative, "
                             f"connectivity {connectivity!r} must be 4 or 8")
    if seg_model is not None:
        for name, v in (("H", H), ("W", W)) if whole else (("tile", tile),):
            if v % 16:
                raise ValueError(f"predict_scene: with a segmentation model {name} must be a multiple of 16 (got {v}): "
                                 "the U-Net halves its input four times")
        unet = _unet(seg_model, batch_stats)
    single = whole or len(ys) * len(xs) == 1
    res = {"grid": (ys, xs)}
    with torch.no_grad():
        if single:
            torch.manual_seed(47)
            out = generator(x)
        else:
            mo = Mosaic(H, W, 3, tile, overlap, x.device)
            for k0, n in mo.batches(batch):
                torch.manual_seed(47)
                mo.add(generator(mo.windows(x, k0, n)), k0)
            out = mo.result()
        if tuple(out.shape) != (1, 3, H, W):
            raise RuntimeError(f"predict_scene: the generator returned {tuple(out.shape)} for a {H} x {W} scene")
        res["output"] = out
        if unet is not None:
            if single:
                z = _flood_logits(unet, out, batch_stats)
                logits = z.interior()[..., :1].permute(0, 3, 1, 2).contiguous()
            else:
                ml = Mosaic(H, W, 1, tile, overlap, x.device)
                for k0, n in ml.batches(batch):
                    ml.add(_flood_logits(unet, ml.windows(out, k0, n), batch_stats), k0)
                logits = ml.result()
            res["flood_logits"] = logits
            res["flood_fraction"] = int(ops.flood_count(logits).cpu()) / (H * W)
            if sieve or elevation is not None or polygons:          # (drainage comes with an elevation)
                from .regions import flood_regions
                regions = flood_regions(logits, "logit", min_region, min_hole, connectivity)     # (1, 0: no sieve)
                res["flood_mask"] = regions.pop("mask")
                res["regions"] = regions
                if sieve:
                    res["flood_fraction_sieved"] = regions["flood_fraction"]
            if elevation is not None:
                from .depth import flood_depth
                depth = flood_depth(res["flood_mask"], elevation, res["regions"], pixel_area)
                res["flood_depth"] = depth.pop("depth")
                res["depth"] = depth
            if polygons:
                from .outline import region_outlines
                res["outlines"] = region_outlines(res["regions"]["labels"], connectivity)
        if drainage:
            add_drainage(res, elevation, flat_rounds)
    return res


def add_drainage(res, elevation, flat_rounds=0):
    """predict_scene's drainage=True on a result `res` of it: "flow" (floodgan.flow.flow_accumulation of the elevation
    with flat_rounds) and, when res holds regions, their table's "max_accumulation" and "pit_pixels", which "flow"
    also carries as "table".  Returns res."""
    from .flow import flow_accumulation, flow_region_table
    flow = flow_accumulation(elevation.contiguous(), flat_rounds=flat_rounds)
    if "regions" in res:
        flow["table"] = flow_region_table(flow, res["regions"])
        res["regions"]["table"].update(flow["table"])
    res["flow"] = flow
    return res


def scene_name(path):
    """the file name of a scene without its directory and extension"""
    return os.path.splitext(os.path.basename(os.fspath(path)))[0]
