"""The flood depth of a scene: the nearest-shore transform and the depth it gives, on the device.

flood_regions answers where a scene floods and over what area; with the scene's elevation this module answers how
deep, by the FwDET scheme: every flood pixel takes the water-surface elevation of its nearest shore pixel, and its
depth is that elevation minus its own, floored at 0.  Not in the reference.  The kernels are csrc/distance.hip
(fg_nearest_seed, fg_shore, fg_flood_depth, fg_depth_table).

  nearest_seed   source -> per pixel the index of the nearest seed pixel and its squared distance
  flood_depth    0 / 1 mask + elevation -> the depth plane, its totals and (with regions) the per-region table

Seed.  A pixel whose class under `kind` (the decisions of floodgan.regions) equals `target`.
Nearest.  The seed at the minimum squared Euclidean distance (y - y')^2 + (x - x')^2; among several, the one with the
smallest index y' W + x'.  The transform is exact and a function of the seed plane alone; a scene without a seed gets
-1 in both planes.
Shore.  A flood pixel (mask > 0.5) with at least one dry 4-neighbour inside the scene; the scene's edge alone makes
no shore.
Depth.  At a flood pixel p with nearest shore pixel s: d = elevation[s] - elevation[p] in fp32, depth = d if d > 0
else 0 (a NaN difference gives 0).  Dry pixels, shore pixels and a scene without a shore have depth 0.
Totals.  In fixed point, q = rint(min(depth, 2^20) * 2^10) per pixel (exact scaling, round-half-even), summed and
maximised as int64 on the device, so they do not depend on the order of the sums; the host divides by 2^10 in fp64.
"""
import numpy as np
import torch

from . import ops
from .regions import check_source, rank_plane, table_columns

Q = 1024.0                       # quanta per unit of depth
DEPTH_TABLE_COLUMNS = ("wet_area", "depth_sum_q", "depth_max_q")


def nearest_seed(src, kind="logit", target=True, dist2=True):
    """(nearest, dist2): int32 [H, W] device tensors -- per pixel the index y' W + x' of the nearest pixel of src's
    class `target` (True flood, False dry) under `kind`, ties to the smallest index, and its squared distance (None
    with dist2=False); -1 everywhere when the scene holds no such pixel.  src: [H, W], [1, 1, H, W], channel 0 of
    [1, C, H, W] or of an NHWC Buf, as floodgan.regions takes it; H, W <= 32768 (ValueError before any launch)."""
    view = check_source(src, kind)
    _, _, H, W = view.shape
    if H > ops.MAX_SEED_SIDE or W > ops.MAX_SEED_SIDE:
        raise ValueError(f"nearest_seed: a scene of {H} x {W}: each side must be at most {ops.MAX_SEED_SIDE} (squared "
                         "distances are int32)")
    near = torch.empty((H, W), dtype=torch.int32, device=view.device)
    d2 = torch.empty((H, W), dtype=torch.int32, device=view.device) if dist2 else None
    return ops.nearest_seed(view, kind, target, near, d2)


def _plane_arg(t, what):
    if not (torch.is_tensor(t) and t.dtype == torch.float32):
        raise ValueError(f"flood_depth: {what} must be a float32 tensor (got {getattr(t, 'dtype', type(t))})")
    if not (t.dim() == 2 or (t.dim() == 4 and t.shape[0] == 1 and t.shape[1] == 1)):
        raise ValueError(f"flood_depth: {what} must be [H, W] or [1, 1, H, W] (got {tuple(t.shape)})")
    return int(t.shape[-2]), int(t.shape[-1])


def _totals(row, count, pixel_area):
    """(max, mean, volume) as fp64 from a {wet_area, sum_q, max_q} row and the number of flood pixels"""
    total = float(row[1]) / Q
    return float(row[2]) / Q, (total / count if count else 0.0), total * float(pixel_area)


def flood_depth(mask, elevation, regions=None, pixel_area=1.0):
    """The depth product of a scene (module docstring): a dict of
      "depth"          fp32 [1, 1, H, W], on the device
      "nearest_shore"  int32 [H, W]: per pixel the index of its nearest shore pixel (-1 without a shore), on the device
      "shore_count"    the number of shore pixels
      "max_depth", "mean_depth", "volume"   fp64: the maximum, the mean over the flood pixels and the sum times
                       pixel_area, all from the fixed-point totals
      "wet_area"       the number of pixels whose depth rounds to at least one quantum
    and, with `regions` (the flood_regions result of this mask, with its table),
      "table"          {wet_area, depth_sum_q, depth_max_q}: int64 numpy of length R, and mean_depth (over the region's
                       area), max_depth, volume: fp64 numpy of length R, rows in the region table's order.
    mask: a 0 / 1 plane as flood_regions returns it, fp32 [H, W] or [1, 1, H, W]; elevation: fp32 of the same H x W on
    the same device.  A type, shape or device mismatch raises ValueError before any launch."""
    H, W = _plane_arg(mask, "the mask")
    if _plane_arg(elevation, "the elevation") != (H, W):
        raise ValueError(f"flood_depth: the elevation is {tuple(elevation.shape)} for a mask of {tuple(mask.shape)}")
    if not mask.is_cuda or mask.device != elevation.device:
        raise ValueError(f"flood_depth: mask and elevation must be on one HIP device (got {mask.device} and "
                         f"{elevation.device})")
    if H < 1 or W < 1 or H > ops.MAX_SEED_SIDE or W > ops.MAX_SEED_SIDE:
        raise ValueError(f"flood_depth: a scene of {H} x {W}: each side must be 1 .. {ops.MAX_SEED_SIDE}")
    if regions is not None:
        if regions.get("table") is None:
            raise ValueError("flood_depth: the regions were computed with table=False")
        if tuple(regions["labels"].shape) != (H, W) or regions["labels"].device != mask.device:
            raise ValueError(f"flood_depth: the regions' labels are {tuple(regions['labels'].shape)} on "
                             f"{regions['labels'].device} for a mask of {H} x {W} on {mask.device}")
    dev = mask.device
    mask, elevation = mask.contiguous(), elevation.contiguous()
    shore = ops.shore(mask, torch.empty((1, 1, H, W), dtype=torch.float32, device=dev))
    near, _ = ops.nearest_seed(shore, "threshold", True, torch.empty((H, W), dtype=torch.int32, device=dev))
    depth = ops.flood_depth(mask, elevation, near, torch.empty((1, 1, H, W), dtype=torch.float32, device=dev))
    scene = ops.depth_table(None, None, depth, torch.empty((1, 3), dtype=torch.int64, device=dev))
    R, rank = rank_plane(regions["labels"], regions["table"]["label"]) if regions is not None else (0, None)
    tab = ops.depth_table(regions["labels"], rank, depth,
                          torch.empty((R, 3), dtype=torch.int64, device=dev)) if R else None
    flooded = int(ops.flood_count(mask.view(1, 1, H, W)).cpu())
    row = scene.cpu().numpy()[0]
    res = {"depth": depth, "nearest_shore": near, "shore_count": int(ops.flood_count(shore).cpu()),
           "wet_area": int(row[0])}
    res["max_depth"], res["mean_depth"], res["volume"] = _totals(row, flooded, pixel_area)
    if regions is not None:
        table = table_columns(tab, DEPTH_TABLE_COLUMNS)
        total = table["depth_sum_q"].astype(np.float64) / Q
        table["mean_depth"] = total / regions["table"]["area"].astype(np.float64)
        table["max_depth"] = table["depth_max_q"].astype(np.float64) / Q
        table["volume"] = total * float(pixel_area)
        res["table"] = table
    return res
