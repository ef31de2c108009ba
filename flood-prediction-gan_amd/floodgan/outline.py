"""The outlines of a scene's flood regions: polygons traced on the device, and the GeoJSON file of them.

flood_regions answers which regions a scene floods and how large; a flood extent is delivered as vector outlines,
one polygon per region with its attributes.  Not in the reference.  The kernels are csrc/outline.hip
(fg_outline_cracks, fg_outline_rings, fg_outline_vertices); everything is integer-exact.

  region_outlines        labels plane -> the rings of every region and their corner vertices
  write_regions_geojson  regions + outlines (+ depth) -> a FeatureCollection of Polygons

Coordinates.  Vertices are grid corners (y, x), 0 <= y <= H, 0 <= x <= W; pixel (y, x) is the square between (y, x)
and (y + 1, x + 1), flood when labels[y, x] >= 0.  Everything outside the scene is dry.
Cracks.  Every side of a flood pixel whose neighbour across it is dry is one directed unit edge, the flood pixel on
its left as drawn with y down: side 0, top, (y, x + 1) -> (y, x); 1, left, (y, x) -> (y + 1, x); 2, bottom,
(y + 1, x) -> (y + 1, x + 1); 3, right, (y + 1, x + 1) -> (y, x + 1).  Outer boundaries therefore run
counter-clockwise in a north-up picture (RFC 7946's exterior rings), holes clockwise.  The key of an edge is
4 (y W + x) + side, an int32: H W must be below 2^29.
Successor.  The edge that starts at an edge's end vertex.  At a saddle (two flood pixels touch diagonally, two edges
start there) the right turn with connectivity 8, which keeps both pixels in one ring, and the left turn with 4.  The
edges fall into disjoint cycles, the rings; at the connectivity the labels were made with, all pixels on the left of a
ring carry one label.
Ring.  start_key: its smallest key (the start edge); label: that of the start edge's pixel; edges: its number of
cracks (its perimeter in pixel sides); signed2 = sum of x_i y_(i+1) - x_(i+1) y_i over its edges; hole = signed2 > 0;
area2 = |signed2|.  A ring is a hole exactly when its start edge is a side 2, else the start edge is a side 0; an outer
ring has start_key = 4 label and every region has exactly one; per region area2(outer) - sum area2(holes) = 2 area.
Vertices.  A ring lists its corners -- the vertices where the arriving and the leaving edge differ in direction -- in
ring order, beginning with the first met from the start edge's start vertex on, that vertex included.  At
connectivity 8 a saddle vertex appears twice in its ring (as with GDAL's -8): such a ring touches itself.
Order.  Rings in ascending (label, start_key): a region's outer ring, then its holes.  The result is a function of the
labels plane and the connectivity alone.

Launches: 4 + 2 ceil(log2 E) for E cracks (1 for E = 0), whatever else the data is; the host reads the device for E,
for the number of rings and for the results.  Memory: 65 bytes per crack (40 of scratch from torch's allocator, 25 of
per-crack results) plus 4 for the ring bases, and 9 bytes per pixel for the side masks, the counts and their prefix
sum; E is about 2 H W at worst (a checkerboard).
"""
import json

import numpy as np
import torch

from . import ops
from .regions import DEPTH_COLUMNS, FLOW_COLUMNS, flow_table

MAX_PIXELS = ops.MAX_OUTLINE_PIXELS
FEATURE_COLUMNS = ("label", "area", "y0", "x0", "y1", "x1")


def _empty():
    i64 = lambda n=0: np.zeros(n, dtype=np.int64)                              # noqa: E731
    return {"edge_count": 0, "ring_count": 0, "vertex_count": 0,
            "rings": {"label": i64(), "start_key": i64(), "edges": i64(), "area2": i64(),
                      "hole": np.zeros(0, dtype=bool), "offset": i64(1)},
            "vertices": np.zeros((0, 2), dtype=np.int32)}


def check_labels(labels, connectivity=8):
    """the argument errors of region_outlines, before any launch; returns (H, W)"""
    if connectivity not in (4, 8):
        raise ValueError(f"region_outlines: connectivity must be 4 or 8 (got {connectivity!r})")
    if not (torch.is_tensor(labels) and labels.dtype == torch.int32):
        raise ValueError("region_outlines: the labels must be an int32 tensor (got "
                         f"{getattr(labels, 'dtype', type(labels))})")
    if not labels.is_cuda or labels.dim() != 2:
        raise ValueError(f"region_outlines: the labels must be an [H, W] plane on a HIP device (got "
                         f"{tuple(labels.shape)} on {labels.device})")
    H, W = int(labels.shape[0]), int(labels.shape[1])
    if H < 1 or W < 1 or H * W >= MAX_PIXELS:
        raise ValueError(f"region_outlines: a scene of {H} x {W} = {H * W} pixels: edge keys are int32, H * W must be "
                         "positive and below 2^29")
    return H, W


def launch_count(edge_count):
    """the kernel launches of region_outlines on a plane with this many cracks"""
    return ops.outline_launches(edge_count)


def region_outlines(labels, connectivity=8):
    """The rings of the flood regions of a labels plane (int32 [H, W] on the device, as flood_regions and
    label_regions return it; module docstring): a dict of
      "edge_count", "ring_count", "vertex_count"   E, N and V
      "rings"     numpy arrays of length N: label, start_key, edges, area2 (int64), hole (bool), and offset (int64,
                  length N + 1); in ascending (label, start_key)
      "vertices"  int32 numpy [V, 2] of (y, x); ring r is vertices[offset[r]:offset[r + 1]].
    `connectivity` is the one the labels were made with.  A plane that is not int32, not on the device or not [H, W],
    H W >= 2^29 and a connectivity other than 4 or 8 raise ValueError before any launch.  65 bytes of device memory
    per crack (40 of them scratch, allocated per call), 4 more for the ring bases and 9 per pixel."""
    H, W = check_labels(labels, connectivity)
    dev = labels.device
    labels = labels.contiguous()
    sides = torch.empty((H, W), dtype=torch.uint8, device=dev)
    count = torch.empty((H, W), dtype=torch.int32, device=dev)
    ops.outline_cracks(labels, sides, count)
    incl = torch.cumsum(count.view(-1), 0, dtype=torch.int32)
    E = int(incl[-1])
    if E == 0:
        return _empty()
    out = {name: torch.empty(E, dtype=torch.int32, device=dev) for name in ("key", "ring", "edges", "corners")}
    out["signed2"] = torch.empty(E, dtype=torch.int64, device=dev)
    out["corner"] = torch.empty(E, dtype=torch.uint8, device=dev)
    ops.outline_rings(labels, sides, incl, connectivity, out)
    # the rings: their start edges in ascending key order, then (stable) by label
    starts = torch.nonzero(out["ring"] == torch.arange(E, dtype=torch.int32, device=dev)).view(-1)
    start_key = out["key"][starts].long()
    label = labels.view(-1)[start_key >> 2].long()
    label, order = torch.sort(label, stable=True)
    starts, start_key = starts[order], start_key[order]
    corners = out["corners"][starts].long()
    offset = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(corners, 0)])
    rings = torch.stack([label, start_key, out["edges"][starts].long(), out["signed2"][starts]]).cpu().numpy()
    offset = offset.cpu().numpy()
    N, V = int(starts.numel()), int(offset[-1])
    base = torch.zeros(E, dtype=torch.int32, device=dev)
    base[starts] = torch.from_numpy(offset[:-1].astype(np.int32)).to(dev)
    vertices = torch.empty((V, 2), dtype=torch.int32, device=dev)
    ops.outline_vertices(out, base, H, W, vertices)
    signed2 = np.ascontiguousarray(rings[3])
    return {"edge_count": E, "ring_count": N, "vertex_count": V,
            "rings": {"label": np.ascontiguousarray(rings[0]), "start_key": np.ascontiguousarray(rings[1]),
                      "edges": np.ascontiguousarray(rings[2]), "area2": np.abs(signed2), "hole": signed2 > 0,
                      "offset": offset},
            "vertices": vertices.cpu().numpy()}


def _position(y, x, transform):
    if transform is None:
        return [int(x), int(y)]
    a, b, c, d, e, f = transform
    x, y = float(x), float(y)
    return [a + x * b + y * c, d + x * e + y * f]


def write_regions_geojson(path, regions, outlines, depth=None, transform=None, flow=None):
    """A GeoJSON FeatureCollection of a flood_regions result and the region_outlines of its labels: one Feature per
    region, in table order; the geometry a Polygon of the region's outer ring, then its holes, each closed by repeating
    its first position.  transform=None: positions are [x, y] as integers; a GDAL-order 6-tuple (a, b, c, d, e, f):
    [a + x b + y c, d + x e + y f] in fp64, written by repr.  Properties: label, area, y0, x0, y1, x1, centroid_y,
    centroid_x, perimeter (the sum of the region's ring `edges`), holes, and with `depth` (flood_depth with these
    regions) wet_area, mean_depth, max_depth, volume, and with `flow` (flow_accumulation with the "table" of these
    regions) max_accumulation, pit_pixels.  Keys are written in a fixed order by the standard json module:
    two writes give the same bytes.  Raises ValueError for regions computed with table=False, for a depth result
    without a table of these regions, and for outlines whose outer rings are not the table's regions.  Returns
    path."""
    tab, cen = regions["table"], regions["centroids"]
    if tab is None:
        raise ValueError("write_regions_geojson: the regions were computed with table=False")
    R = len(tab["label"])
    dtab = None
    if depth is not None:
        dtab = depth.get("table")
        if dtab is None or len(dtab["wet_area"]) != R:
            raise ValueError("write_regions_geojson: the depth result holds no table of these regions (flood_depth "
                             "with regions=)")
    ftab = flow_table(flow, R, "write_regions_geojson")
    if transform is not None:
        transform = tuple(float(v) for v in transform)
        if len(transform) != 6:
            raise ValueError(f"write_regions_geojson: the transform is a GDAL-order 6-tuple (got {len(transform)} values)")
    rings, verts = outlines["rings"], outlines["vertices"]
    outer = np.flatnonzero(~rings["hole"])
    if len(outer) != R or not np.array_equal(rings["label"][outer], tab["label"]):
        raise ValueError("write_regions_geojson: the outlines' outer rings are not the regions of the table (outlines "
                         "of another labels plane?)")
    # a region's rings are the run from its outer ring to the next one
    ends = np.append(outer[1:], len(rings["label"]))
    features = []
    for r in range(R):
        run = range(int(outer[r]), int(ends[r]))
        if any(rings["label"][k] != tab["label"][r] for k in run):
            raise ValueError(f"write_regions_geojson: a ring of another label among those of region {tab['label'][r]}")
        coords = []
        for k in run:
            pts = [_position(y, x, transform) for y, x in verts[rings["offset"][k]:rings["offset"][k + 1]].tolist()]
            coords.append(pts + pts[:1])
        props = {c: int(tab[c][r]) for c in FEATURE_COLUMNS}
        props["centroid_y"], props["centroid_x"] = float(cen[r, 0]), float(cen[r, 1])
        props["perimeter"] = int(sum(int(rings["edges"][k]) for k in run))
        props["holes"] = len(run) - 1
        if dtab is not None:
            props["wet_area"] = int(dtab["wet_area"][r])
            for c in DEPTH_COLUMNS[1:]:
                props[c] = float(dtab[c][r])
        if ftab is not None:
            for c in FLOW_COLUMNS:
                props[c] = int(ftab[c][r])
        features.append({"type": "Feature", "properties": props,
                         "geometry": {"type": "Polygon", "coordinates": coords}})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": features}, f)
        f.write("\n")
    return path
