"""Where the water runs: D8 flow directions, flow accumulation, basins and path lengths of a scene's elevation, on
the device.

flood_regions answers where a scene floods and flood_depth how deep; this module answers the next question asked of
the same elevation: which way every pixel drains, how many pixels drain through it, and into which pit.  Not in the
reference, which cuts its flow-accumulation channel from maps made in a desktop GIS.  The kernels are csrc/flow.hip
(fg_flow_directions, fg_flow_flats, fg_flow_accumulate, fg_flow_region_table).

  flow_directions    elevation -> the uint8 direction plane and its counts
  flow_accumulation  elevation or direction plane -> accumulation, basin and length
  render_flow        accumulation -> an fp32 plane in [0, 1] for pictures

Data.  A pixel is data when its elevation is finite; NaN and the infinities are nodata.  What lies outside the scene is
unknown and never a neighbour.
Codes.  k = 0 .. 7: E, SE, S, SW, W, NW, N, NE, (dy, dx) = NEIGHBOURS[k]; 8 (PIT): a data pixel that drains nowhere;
255 (NODATA).
Direction.  For a data pixel p and each data neighbour n_k inside the scene, d_k = z[p] - z[n_k] in fp32; only d_k > 0
qualifies; the steepness key is c_k (double) d_k (double) d_k, c_k = 2 for a cardinal and 1 for a diagonal k (the
squares of d / 1 and d / sqrt(2): exact in fp64, so the device and numpy agree bit for bit); p takes the largest key,
among equal keys the smallest k.
Flats.  flat_rounds = R rounds (0 .. 32768) of a breadth-first wave: in round r a pixel that is still a pit takes the
direction of its first neighbour, in the order 0, 2, 4, 6, 1, 3, 5, 7, of exactly its elevation that was directed at
the end of round r - 1.  Flats without an outlet, and the parts of a flat more than R steps from one, stay pits.
Receiver.  The neighbour a direction names.  In a direction plane a caller passes, a byte that is neither 0 .. 8 nor
255, a neighbour outside the scene and a nodata neighbour make the pixel a pit.
Accumulation, basin, length.  acc[p]: the data pixels whose path passes through p, itself included (0 on nodata);
basin[p]: the index y W + x of the pit p's path ends in (-1 on nodata); length[p]: the steps to it (-1 on nodata).

The number of kernel launches depends on H, W and flat_rounds, never on the data.
"""
import numpy as np
import torch

from . import ops

NEIGHBOURS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))
PIT, NODATA = 8, 255
MAX_PIXELS = 2 ** 31 - 1
FLOW_TABLE_COLUMNS = ("max_accumulation", "pit_pixels")


def check_flat_rounds(flat_rounds):
    """flat_rounds as an int, or ValueError: an integer of 0 .. 32768"""
    if isinstance(flat_rounds, bool) or not isinstance(flat_rounds, (int, np.integer)):
        raise ValueError(f"flow: flat_rounds must be an integer (got {flat_rounds!r})")
    if flat_rounds < 0 or flat_rounds > ops.MAX_FLAT_ROUNDS:
        raise ValueError(f"flow: flat_rounds {flat_rounds} must be 0 .. {ops.MAX_FLAT_ROUNDS}")
    return int(flat_rounds)


def _check_plane(t, what, dtype):
    """the argument errors of a plane, before any launch; returns (H, W)"""
    if not (torch.is_tensor(t) and t.dtype == dtype):
        raise ValueError(f"flow: {what} must be a {dtype} tensor (got {getattr(t, 'dtype', type(t))})")
    if not (t.dim() == 2 or (t.dim() == 4 and t.shape[0] == 1 and t.shape[1] == 1)):
        raise ValueError(f"flow: {what} must be [H, W] or [1, 1, H, W] (got {tuple(t.shape)})")
    H, W = int(t.shape[-2]), int(t.shape[-1])
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"flow: a scene of {H} x {W} = {H * W} pixels: indices are int32, H * W must be positive and "
                         "below 2^31")
    if not t.is_cuda:
        raise ValueError(f"flow: {what} must be on a HIP device (got {t.device}); there is no CPU path")
    if not t.is_contiguous():
        raise ValueError(f"flow: {what} must be contiguous (strides {tuple(t.stride())})")
    return H, W


def _counts(directions):
    """(pit_count, nodata_count) of a direction plane: one device -> host read"""
    host = torch.stack([(directions == PIT).sum(), (directions == NODATA).sum()]).cpu()
    return int(host[0]), int(host[1])


def flow_directions(elevation, flat_rounds=0):
    """The direction product of an elevation (module docstring): a dict of
      "directions"     uint8 [H, W], on the device: 0 .. 7, 8 a pit, 255 nodata
      "pit_count", "nodata_count"   the number of pits and of nodata pixels of that plane
      "flat_directed"  int32 numpy [flat_rounds]: entry r - 1 is the number of pixels round r of the flat wave directed.
    elevation: contiguous fp32 [H, W] or [1, 1, H, W] on the device.  A type, shape, device or flat_rounds error raises
    ValueError before any launch."""
    R = check_flat_rounds(flat_rounds)
    H, W = _check_plane(elevation, "the elevation", torch.float32)
    dev = elevation.device
    d = ops.flow_directions(elevation, torch.empty((H, W), dtype=torch.uint8, device=dev))
    directed = np.zeros(0, dtype=np.int32)
    if R:
        d, counts = ops.flow_flats(elevation, d, R, torch.empty((H, W), dtype=torch.uint8, device=dev),
                                   torch.empty(R, dtype=torch.int32, device=dev))
        directed = counts.cpu().numpy()
    pits, nodata = _counts(d)
    return {"directions": d, "pit_count": pits, "nodata_count": nodata, "flat_directed": directed}


def flow_accumulation(elevation=None, *, directions=None, flat_rounds=0):
    """The drainage product of a scene (module docstring), from exactly one of `elevation` (as flow_directions takes
    it, with flat_rounds) and `directions` (a contiguous uint8 [H, W] or [1, 1, H, W] device plane, for example one
    that was hydrologically conditioned elsewhere; flat_rounds must then be 0).  flow_directions' dict ("flat_directed"
    empty for a plane that was passed), and
      "accumulation", "basin", "length"   int32 [H, W], on the device
      "rounds"         K = ceil(log2 max(H W, 2)), the doubling rounds that were run."""
    if (elevation is None) == (directions is None):
        raise ValueError("flow_accumulation: pass exactly one of elevation and directions")
    R = check_flat_rounds(flat_rounds)
    if directions is not None:
        if R:
            raise ValueError("flow_accumulation: flat_rounds resolves the flats of an elevation; a direction plane is "
                             "taken as it is")
        H, W = _check_plane(directions, "the direction plane", torch.uint8)
        d = directions.view(H, W)
        pits, nodata = _counts(d)
        res = {"directions": d, "pit_count": pits, "nodata_count": nodata, "flat_directed": np.zeros(0, dtype=np.int32)}
    else:
        res = flow_directions(elevation, R)
        d = res["directions"]
        H, W = d.shape
    acc, basin, length = (torch.empty((H, W), dtype=torch.int32, device=d.device) for _ in range(3))
    ops.flow_accumulate(d, acc, basin, length)
    res.update(accumulation=acc, basin=basin, length=length, rounds=ops.flow_rounds(H, W))
    return res


def flow_region_table(flow, regions):
    """{max_accumulation, pit_pixels}: int64 numpy of length R, rows in the region table's order -- per region of a
    flood_regions result (with its table) the largest accumulation among its pixels and the number of its pixels that
    are pits of the flow_accumulation result `flow`."""
    from .regions import rank_plane, table_columns
    if regions.get("table") is None:
        raise ValueError("flow_region_table: the regions were computed with table=False")
    labels, acc = regions["labels"], flow["accumulation"]
    if tuple(labels.shape) != tuple(acc.shape) or labels.device != acc.device:
        raise ValueError(f"flow_region_table: the regions' labels are {tuple(labels.shape)} on {labels.device} for a "
                         f"flow of {tuple(acc.shape)} on {acc.device}")
    R, rank = rank_plane(labels, regions["table"]["label"])
    tab = ops.flow_region_table(labels, rank, acc, flow["directions"],
                                torch.empty((R, 2), dtype=torch.int64, device=acc.device)) if R else None
    return table_columns(tab, FLOW_TABLE_COLUMNS)


def render_flow(acc, vmax=None):
    """fp32 plane in [0, 1] of the shape of acc (an integer tensor, any device): log2(max(acc, 1)) / log2(max(vmax,
    2)), clamped to 1; vmax defaults to the scene's data-pixel count (the pixels with acc > 0), the largest value an
    accumulation can take."""
    if not (torch.is_tensor(acc) and not acc.dtype.is_floating_point and acc.dtype != torch.bool):
        raise ValueError(f"render_flow: the accumulation must be an integer tensor (got {getattr(acc, 'dtype', type(acc))})")
    if vmax is None:
        vmax = int((acc > 0).sum())
    elif not vmax > 0:
        raise ValueError(f"render_flow: vmax {vmax!r} must be positive")
    num = torch.log2(torch.clamp(acc, min=1).to(torch.float32))
    den = torch.log2(torch.tensor(float(max(vmax, 2)), dtype=torch.float32, device=acc.device))
    return torch.clamp(num / den, 0.0, 1.0)
