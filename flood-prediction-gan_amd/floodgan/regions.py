"""The flood regions of a scene: connected-component labelling, the sieve and the region table, on the device.

predict_scene ends at a plane of blended logits; a flood map is that plane thresholded, cleaned of specks and
pin-holes below a minimum mapping unit, and read as a list of regions: which areas flood, how large, and where.  Not
in the reference.  The kernels are csrc/regions.hip (fg_regions_label, fg_regions_stats, fg_regions_table,
fg_regions_apply); everything is integer-exact.

  label_regions      source -> int32 [H, W] canonical labels of the flood (or the dry) class
  flood_regions      source -> the sieved mask, its labels, the region table and the centroids
  write_regions_csv  the table as a CSV file

Mask.  kind "logit": a pixel is flood when sigmoid(z) > 0.5 in fp32, the decision of fg_mask_confusion (+0, -0 and
NaN are dry, +inf is flood); kind "threshold": when x > 0.5.
Components.  `connectivity` (8, the default, or 4) is that of the flood class; the dry class always takes the
complementary one, so that a diagonal chain of flood pixels that is one region at 8 also separates the dry pixels
on its two sides, and one that is not a region at 4 does not.
Label.  A member pixel's label is the index y * W + x of its component's first pixel in row-major order (the
smallest index of the component); the other class gets -1.  The labels depend on the mask alone.
Sieve.  (1) Flood components with area < min_region become dry.  (2) On that result, dry components with area <
min_hole that hold no pixel of the scene's first or last row or column become flood; dry regions that touch the border
are background and are never filled.  min_region <= 1 and min_hole <= 0 switch the step off.
Regions.  The flood components of the final mask, labelled again (filled holes can join regions), in ascending label
order: the row-major order of their first pixels.  Per region label, area, y0, x0, y1, x1 (inclusive box), sum_y,
sum_x as int64; the centroid is sum / area in fp64 on the host.

The number of kernel launches depends on H, W and the options, never on the data; the host reads the device once for
the number of regions (and once each for the counts and the fraction it returns).
"""
import numpy as np
import torch

from . import ops
from .plans import Buf

COLUMNS = ("label", "area", "y0", "x0", "y1", "x1", "sum_y", "sum_x")
MAX_PIXELS = 2 ** 31 - 1


def check_source(src, kind, min_region=1, min_hole=0, connectivity=8):
    """the option errors, before any launch; returns the [1, C, H, W] view the kernels read"""
    if kind not in ops.REGION_KINDS:
        raise ValueError(f"regions: kind must be one of {sorted(ops.REGION_KINDS)} (got {kind!r})")
    if connectivity not in (4, 8):
        raise ValueError(f"regions: connectivity must be 4 or 8 (got {connectivity!r})")
    if min_region < 0 or min_hole < 0:
        raise ValueError(f"regions: min_region {min_region} and min_hole {min_hole} must not be negative")
    t = src.t if isinstance(src, Buf) else src
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise ValueError("regions: the source must be a float32 tensor on a HIP device "
                         f"(got {getattr(t, 'dtype', type(t))} on {getattr(t, 'device', 'the host')})")
    if not isinstance(src, Buf) and not (src.dim() == 2 or (src.dim() == 4 and src.shape[0] == 1)):
        raise ValueError(f"regions: need [H, W], [1, C, H, W] or an NHWC Buf of one image (got {tuple(src.shape)})")
    if isinstance(src, Buf) and src.n != 1:
        raise ValueError(f"regions: an NHWC Buf of one image (got {src.n})")
    H, W = (src.h, src.w) if isinstance(src, Buf) else (int(src.shape[-2]), int(src.shape[-1]))
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"regions: a scene of {H} x {W} = {H * W} pixels: labels are int32 pixel indices, H * W must "
                         "be positive and below 2^31")
    return ops.region_source(src)


def _label(view, kind, target, connectivity):
    _, _, H, W = view.shape
    return ops.regions_label(view, kind, target, connectivity,
                             torch.empty((H, W), dtype=torch.int32, device=view.device))


def label_regions(src, kind="logit", target=True, connectivity=8):
    """int32 [H, W] device tensor: the canonical labels of the flood class (target=True) or of the dry class
    (target=False, labelled with the complementary connectivity) of src -- [H, W], [1, 1, H, W], channel 0 of
    [1, C, H, W] or of an NHWC Buf -- and -1 on the other class (module docstring)."""
    return _label(check_source(src, kind, 1, 0, connectivity), kind, target, connectivity)


def region_table(labels):
    """(R, table) of a labels plane: table an int64 [R, 8] device tensor in COLUMNS order, rows in ascending label
    order; one device -> host read (the number of roots).  R = 0 gives an empty table without a launch."""
    R, rank = rank_plane(labels)
    table = torch.empty((R, 8), dtype=torch.int64, device=labels.device)
    if R:
        ops.regions_table(labels, rank, table)
    return R, table


def rank_plane(labels, roots=None):
    """(R, rank): rank an int32 [H, W] device plane that holds 0 .. R - 1 at the R roots of a labels plane, in ascending
    order (None when R = 0).  roots: their indices (int64 numpy) where the caller has them; else they are found here,
    with one device -> host read (their number)."""
    dev = labels.device
    if roots is None:
        roots = torch.nonzero(labels.view(-1) == torch.arange(labels.numel(), dtype=torch.int32, device=dev)).view(-1)
    else:
        roots = torch.from_numpy(np.ascontiguousarray(roots)).to(dev)
    R = int(roots.numel())
    if not R:
        return 0, None
    rank = torch.empty_like(labels)
    rank.view(-1)[roots] = torch.arange(R, dtype=torch.int32, device=dev)
    return R, rank


def table_columns(table, names):
    """{name: int64 numpy [R]} of an int64 [R, len(names)] device table (one device -> host read); None: no rows"""
    cols = table.cpu().numpy() if table is not None else np.zeros((0, len(names)), dtype=np.int64)
    return {name: np.ascontiguousarray(cols[:, j]) for j, name in enumerate(names)}


def flood_regions(src, kind="logit", min_region=1, min_hole=0, connectivity=8, table=True):
    """The flood-extent product of a scene (module docstring): a dict of
      "mask"            fp32 [1, 1, H, W] of 0 / 1: the final mask, on the device
      "labels"          int32 [H, W]: the canonical labels of the final mask's flood class, on the device
      "count"           R, the number of regions
      "table"           {label, area, y0, x0, y1, x1, sum_y, sum_x}: int64 numpy arrays of length R (None with
                        table=False, which skips the table launches)
      "centroids"       fp64 [R, 2] numpy: (sum_y / area, sum_x / area) (None with table=False)
      "removed", "filled"   the flood components the sieve removed and the holes it filled
      "flood_fraction"  the share of flood pixels of the final mask."""
    min_region, min_hole = int(min_region), int(min_hole)
    view = check_source(src, kind, min_region, min_hole, connectivity)
    _, _, H, W = view.shape
    dev = view.device
    cap = lambda v: min(v, MAX_PIXELS)                                     # noqa: E731  (an area never exceeds it)
    mask = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
    counts = torch.zeros((2, 2), dtype=torch.int64, device=dev)           # rows: removed, filled
    labels = _label(view, kind, True, connectivity)
    sieve_flood, sieve_dry = min_region > 1, min_hole > 0
    area = border = None
    if sieve_flood or sieve_dry:
        area = torch.empty((H, W), dtype=torch.int32, device=dev)
        border = torch.empty((H, W), dtype=torch.int32, device=dev)
    if sieve_flood:
        ops.regions_stats(labels, area, border)
    ops.regions_apply(labels, area if sieve_flood else None, border if sieve_flood else None, "remove",
                      cap(min_region), mask, counts[0])
    if sieve_dry:
        dry = _label(mask, "threshold", False, connectivity)
        ops.regions_stats(dry, area, border)
        ops.regions_apply(dry, area, border, "fill", cap(min_hole), mask, counts[1])
    if sieve_flood or sieve_dry:
        labels = _label(mask, "threshold", True, connectivity)
    res = {"mask": mask, "labels": labels, "table": None, "centroids": None}
    if table:
        R, tab = region_table(labels)
        res["table"] = table_columns(tab, COLUMNS)
        a = res["table"]["area"].astype(np.float64)
        res["centroids"] = np.stack([res["table"]["sum_y"] / a, res["table"]["sum_x"] / a], axis=1)
    else:
        R = int((labels.view(-1) == torch.arange(H * W, dtype=torch.int32, device=dev)).sum())
    host = counts.cpu()
    res["count"] = R
    res["removed"], res["filled"] = int(host[0, 0]), int(host[1, 0])
    res["flood_fraction"] = int(ops.flood_count(mask).cpu()) / (H * W)
    return res


DEPTH_COLUMNS = ("wet_area", "mean_depth", "max_depth", "volume")


FLOW_COLUMNS = ("max_accumulation", "pit_pixels")


def flow_table(flow, R, who):
    """the {max_accumulation, pit_pixels} table of a flow result for R regions, or None without a flow result"""
    if flow is None:
        return None
    ftab = flow.get("table")
    if ftab is None or len(ftab["max_accumulation"]) != R:
        raise ValueError(f"{who}: the flow result holds no table of these regions (floodgan.flow.flow_region_table)")
    return ftab


def write_regions_csv(path, regions, depth=None, flow=None):
    """One header line (COLUMNS, then centroid_y, centroid_x) and one line per region of a flood_regions result;
    integers as integers, the centroids by repr (they read back to the same fp64).  With `depth` (a
    floodgan.depth.flood_depth result computed with these regions) the lines gain DEPTH_COLUMNS: wet_area as an
    integer, the others by repr.  With `flow` (a floodgan.flow.flow_accumulation result that carries the "table" of
    these regions) they gain FLOW_COLUMNS after those, as integers.  Returns path."""
    tab, cen = regions["table"], regions["centroids"]
    if tab is None:
        raise ValueError("write_regions_csv: the regions were computed with table=False")
    head, dtab = COLUMNS + ("centroid_y", "centroid_x"), None
    ftab = flow_table(flow, len(tab["label"]), "write_regions_csv")
    if depth is not None:
        dtab = depth.get("table")
        if dtab is None or len(dtab["wet_area"]) != len(tab["label"]):
            raise ValueError("write_regions_csv: the depth result holds no table of these regions (flood_depth with "
                             "regions=)")
        head = head + DEPTH_COLUMNS
    if ftab is not None:
        head = head + FLOW_COLUMNS
    with open(path, "w") as f:
        f.write(",".join(head) + "\n")
        for r in range(len(tab["label"])):
            cells = [str(int(tab[c][r])) for c in COLUMNS] + [repr(float(cen[r, 0])), repr(float(cen[r, 1]))]
            if dtab is not None:
                cells += [str(int(dtab["wet_area"][r]))] + [repr(float(dtab[c][r])) for c in DEPTH_COLUMNS[1:]]
            if ftab is not None:
                cells += [str(int(ftab[c][r])) for c in FLOW_COLUMNS]
            f.write(",".join(cells) + "\n")
    return path
