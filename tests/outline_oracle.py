"""Plain-Python oracle of floodgan.outline: a sequential crack tracer written from the semantics (no device).

Vertices are grid corners (y, x), 0 <= y <= H, 0 <= x <= W; pixel (y, x) is the square between (y, x) and
(y + 1, x + 1) and is flood when labels[y, x] >= 0; everything outside the scene is dry.  A crack is a side of a flood
pixel whose neighbour across it is dry, directed with the flood pixel on its left:
  side 0, top     (y, x + 1) -> (y, x)          side 2, bottom  (y + 1, x) -> (y + 1, x + 1)
  side 1, left    (y, x) -> (y + 1, x)          side 3, right   (y + 1, x + 1) -> (y, x + 1)
with the key 4 (y W + x) + side.  The successor of a crack is the crack that starts at its end vertex; at a saddle
(two start there) the right turn at connectivity 8, the left turn at 4.  The tracer gathers the cracks, takes the
smallest key not yet visited as a ring's start and walks the successors until it is back.

rebuild_mask is independent of the tracing: it fills the polygons a result lists by the parity of their vertical
segments."""
import numpy as np

# per side: the start vertex's offset from the pixel, and the direction of travel
START = ((0, 1), (0, 0), (1, 0), (1, 1))
STEP = ((0, -1), (1, 0), (0, 1), (-1, 0))
# the pixel on the far side of a side, relative to its own (the dry one)
OUT = ((-1, 0), (0, -1), (1, 0), (0, 1))


def crack_keys(flood):
    """the keys of all cracks of a boolean [H, W] mask, ascending (int64)"""
    p = np.pad(flood, 1)
    dry = [~p[:-2, 1:-1], ~p[1:-1, :-2], ~p[2:, 1:-1], ~p[1:-1, 2:]]           # above, left, below, right
    return np.flatnonzero(np.stack([flood & d for d in dry], axis=-1).reshape(-1)).astype(np.int64)


def outlines(labels, connectivity=8):
    """the oracle of floodgan.outline.region_outlines on an int32 [H, W] numpy labels plane: the same dict"""
    assert connectivity in (4, 8)
    labels = np.asarray(labels)
    H, W = labels.shape
    flood = labels >= 0
    P = W + 2
    wet = np.pad(flood, 1).reshape(-1).tolist()                                # wet[(y + 1) * P + x + 1]
    keys = crack_keys(flood)
    is_crack = bytearray(4 * H * W)
    for k in keys.tolist():
        is_crack[k] = 1
    seen = bytearray(4 * H * W)
    rings = []
    for start in keys.tolist():
        if seen[start]:
            continue
        k, dirs, starts, signed2 = start, [], [], 0
        while not seen[k]:
            seen[k] = 1
            s, i = k & 3, k >> 2
            y, x = divmod(i, W)
            vy, vx = y + START[s][0], x + START[s][1]
            hy, hx = STEP[s]
            signed2 += vx * (vy + hy) - (vx + hx) * vy
            dirs.append(s)
            starts.append((vy, vx))
            # the two pixels ahead of the end vertex: a beside the flood pixel, b beside the dry one
            ay, ax = y + hy, x + hx
            by, bx = ay + OUT[s][0], ax + OUT[s][1]
            a, b = wet[(ay + 1) * P + ax + 1], wet[(by + 1) * P + bx + 1]
            if a and b:
                turn = "right"
            elif a:
                turn = "straight"
            elif b:
                turn = "right" if connectivity == 8 else "left"               # the saddle
            else:
                turn = "left"
            if turn == "right":
                k = 4 * (by * W + bx) + (s + 3) % 4
            elif turn == "straight":
                k = 4 * (ay * W + ax) + s
            else:
                k = 4 * i + (s + 1) % 4
            assert is_crack[k], (start, k)
        assert k == start, (start, k)                                          # the walk closes where it began
        n = len(dirs)
        corners = [starts[t] for t in range(n) if dirs[t - 1] != dirs[t]]
        rings.append({"label": int(labels[(start >> 2) // W, (start >> 2) % W]), "start_key": start, "edges": n,
                      "signed2": signed2, "vertices": corners})
    rings.sort(key=lambda r: (r["label"], r["start_key"]))
    return pack(rings, len(keys))


def pack(rings, edge_count):
    """a list of ring dicts (label, start_key, edges, signed2, vertices) as region_outlines' result"""
    counts = [len(r["vertices"]) for r in rings]
    col = lambda name: np.array([r[name] for r in rings], dtype=np.int64)                   # noqa: E731
    signed2 = col("signed2")
    verts = [v for r in rings for v in r["vertices"]]
    return {"edge_count": edge_count, "ring_count": len(rings), "vertex_count": len(verts),
            "rings": {"label": col("label"), "start_key": col("start_key"), "edges": col("edges"),
                      "area2": np.abs(signed2), "hole": signed2 > 0,
                      "offset": np.concatenate(([0], np.cumsum(counts))).astype(np.int64)},
            "vertices": np.array(verts, dtype=np.int32).reshape(-1, 2)}


def rebuild_mask(out, H, W):
    """the boolean [H, W] mask the rings of an outlines result enclose, by parity: every vertical segment
    (y0, x) - (y1, x) of every ring toggles D[min(y0, y1) .. max(y0, y1) - 1, x], and the mask is the running XOR of D
    along x"""
    off, a = np.asarray(out["rings"]["offset"]), np.asarray(out["vertices"]).astype(np.int64)
    if len(a) == 0:
        return np.zeros((H, W), dtype=bool)
    nxt = np.arange(1, len(a) + 1)
    nxt[off[1:] - 1] = off[:-1]                                                # a ring's last vertex joins its first
    b = a[nxt]
    up = a[:, 1] == b[:, 1]
    # toggling rows min .. max - 1 of a column is a toggle at min and one at max, then a running XOR down the rows
    T = np.zeros((H + 1, W + 1), dtype=np.int64)
    np.add.at(T, (a[up, 0], a[up, 1]), 1)
    np.add.at(T, (b[up, 0], b[up, 1]), 1)
    D = np.cumsum(T, axis=0)[:H] % 2
    return (np.cumsum(D, axis=1)[:, :W] % 2).astype(bool)
