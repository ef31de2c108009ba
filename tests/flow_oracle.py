"""Plain numpy / Python oracle of floodgan.flow: D8 directions, the flat wave, receivers, accumulation, basin and
length, written from the semantics (no device, no doubling).

Directions: the fp64 key c d d of the fp32 drop d, neighbour by neighbour on shifted planes.  Flats: round by round,
each round reading a copy of the previous plane.  Accumulation: in-degree peeling (leaves first), then basin and length
in the reverse order (pits first).  follow(p) walks one path step by step."""
import numpy as np

import regions_oracle as RO

NEIGHBOURS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))
FLAT_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)
PIT, NODATA = 8, 255


def rounds(H, W):
    """ceil(log2 max(H W, 2)) in integers"""
    return (max(H * W, 2) - 1).bit_length()


def _shifted(a, k, fill):
    """n[y, x] = a[y + dy, x + dx] of neighbour k, `fill` outside the scene"""
    H, W = a.shape
    dy, dx = NEIGHBOURS[k]
    p = np.full((H + 2, W + 2), fill, dtype=a.dtype)
    p[1:-1, 1:-1] = a
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def directions(z):
    """uint8 [H, W]: the D8 code of every pixel of the fp32 elevation z"""
    z = np.asarray(z)
    assert z.dtype == np.float32 and z.ndim == 2
    data = np.isfinite(z)
    best = np.full(z.shape, PIT, dtype=np.uint8)
    key = np.zeros(z.shape, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(8):
            zn = _shifted(z, k, np.float32(np.nan))
            d = (z - zn).astype(np.float32)                       # one fp32 subtraction
            ok = data & np.isfinite(zn) & (d > 0)
            dd = d.astype(np.float64)
            s = np.where(ok, (1.0 if k % 2 else 2.0) * dd * dd, 0.0)
            win = s > key                                         # strictly: ties stay with the smaller k
            key[win] = s[win]
            best[win] = k
    best[~data] = NODATA
    return best


def flats(z, d, R):
    """(directions after R rounds of the flat wave, int32 [R] pixels directed per round)"""
    z, d = np.asarray(z), np.array(d, dtype=np.uint8)
    counts = np.zeros(R, dtype=np.int32)
    for r in range(R):
        prev = d.copy()
        open_ = prev == PIT
        for k in FLAT_ORDER:
            zn, cn = _shifted(z, k, np.float32(np.nan)), _shifted(prev, k, np.uint8(NODATA))
            take = open_ & (cn < 8) & (zn == z)
            d[take] = k
            open_ &= ~take
        counts[r] = int((d != prev).sum())
    return d, counts


def receivers(d):
    """int32 [H W]: the index of the neighbour each direction names; -1 for pits and nodata, and for a byte that is no
    code, a neighbour outside the scene and a nodata neighbour (which make a pit)"""
    d = np.asarray(d)
    H, W = d.shape
    recv = np.full(H * W, -1, dtype=np.int32)
    for y in range(H):
        for x in range(W):
            c = int(d[y, x])
            if c < 8:
                yn, xn = y + NEIGHBOURS[c][0], x + NEIGHBOURS[c][1]
                if 0 <= yn < H and 0 <= xn < W and d[yn, xn] != NODATA:
                    recv[y * W + x] = yn * W + xn
    return recv


def accumulate(d):
    """(acc, basin, length): int32 [H, W] each, from a direction plane, by in-degree peeling"""
    d = np.asarray(d)
    H, W = d.shape
    n = H * W
    recv = receivers(d).tolist()
    data = (d.ravel() != NODATA).tolist()
    indeg = [0] * n
    for r in recv:
        if r >= 0:
            indeg[r] += 1
    acc = [1 if v else 0 for v in data]
    ready = [p for p in range(n) if data[p] and indeg[p] == 0]
    order = []
    while ready:
        p = ready.pop()
        order.append(p)
        r = recv[p]
        if r >= 0:
            acc[r] += acc[p]
            indeg[r] -= 1
            if indeg[r] == 0:
                ready.append(r)
    assert len(order) == sum(data), "the receivers hold a cycle"
    basin, length = [-1] * n, [-1] * n
    for p in reversed(order):                                     # a receiver comes before the pixels that drain to it
        r = recv[p]
        basin[p], length[p] = (p, 0) if r < 0 else (basin[r], length[r] + 1)
    return tuple(np.array(a, dtype=np.int32).reshape(H, W) for a in (acc, basin, length))


def follow(recv, p):
    """(the pit p's path ends in, the number of steps), walking step by step"""
    steps = 0
    while recv[p] >= 0:
        p = int(recv[p])
        steps += 1
        assert steps <= len(recv), "a cycle"
    return p, steps


def flow(z, R=0):
    """the oracle of floodgan.flow.flow_accumulation on an fp32 elevation"""
    d, directed = flats(z, directions(z), R)
    acc, basin, length = accumulate(d)
    return {"directions": d, "pit_count": int((d == PIT).sum()), "nodata_count": int((d == NODATA).sum()),
            "flat_directed": directed, "accumulation": acc, "basin": basin, "length": length,
            "rounds": rounds(*d.shape)}


def region_table(labels, acc, d):
    """{max_accumulation, pit_pixels}: int64 [R], rows in ascending label order"""
    member = labels >= 0
    ids, inv = np.unique(labels[member], return_inverse=True)
    mx, pits = np.zeros(len(ids), dtype=np.int64), np.zeros(len(ids), dtype=np.int64)
    np.maximum.at(mx, inv, acc[member].astype(np.int64))
    np.add.at(pits, inv, (d[member] == PIT).astype(np.int64))
    return {"max_accumulation": mx, "pit_pixels": pits}


def render(acc, vmax=None):
    """fp32 log2(max(acc, 1)) / log2(max(vmax, 2)), clamped to 1"""
    vmax = int((acc > 0).sum()) if vmax is None else vmax
    num = np.log2(np.maximum(acc, 1).astype(np.float32))
    return np.minimum(num / np.log2(np.float32(max(vmax, 2))), np.float32(1)).astype(np.float32)


# ---- the elevation patterns (fp32 [H, W])

def _rng(H, W, seed):
    return np.random.default_rng(seed + 1000 * H + W)


def _trench(mask):
    """a one-pixel path mask walked from (0, 0) through its 4-neighbours: the trench descends one unit per step and
    ends in the single pit; everything off the path is a wall above the trench's top"""
    H, W = mask.shape
    path, seen = [(0, 0)], {(0, 0)}
    while True:
        y, x = path[-1]
        nxt = [(y + dy, x + dx) for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0))
               if 0 <= y + dy < H and 0 <= x + dx < W and mask[y + dy, x + dx] and (y + dy, x + dx) not in seen]
        if not nxt:
            break
        path.append(nxt[0])
        seen.add(nxt[0])
    z = np.full((H, W), float(len(path) + 7), dtype=np.float32)
    for step, (y, x) in enumerate(path):
        z[y, x] = len(path) - 1 - step
    return z


def cone(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return ((y - H // 2) ** 2 + (x - W // 2) ** 2).astype(np.float32)


def lowpass(H, W, seed=7):
    """uniform noise under a box filter of radius max(1, min(H, W) // 12), stretched to [0, 1]"""
    r = max(1, min(H, W) // 12)
    n = _rng(H, W, seed).random((H + 2 * r, W + 2 * r))
    c = np.cumsum(np.cumsum(np.pad(n, ((1, 0), (1, 0))), axis=0), axis=1)
    k = 2 * r + 1
    s = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
    lo, hi = s.min(), s.max()
    return (s - lo) / (hi - lo) if hi > lo else np.zeros((H, W))


def terraces(H, W):
    return np.floor(8 * lowpass(H, W)).astype(np.float32)


def noise(H, W):
    z = _rng(H, W, 3).random((H, W), dtype=np.float32)
    if W > 1:                                                     # neighbours one ulp apart, up and down
        z[::3, 1::4] = np.nextafter(z[::3, 0:W - 1:4], np.float32(2))
    if H > 1:
        z[1::5, ::7] = np.nextafter(z[0:H - 1:5, ::7], np.float32(-1))
    return z


def holes(H, W):
    z = noise(H, W)
    z[H // 3:H // 3 + max(1, H // 6), W // 4:W // 4 + max(1, W // 5)] = np.nan
    z[H // 2, (2 * W) // 3] = np.inf
    z[(3 * H) // 4, W // 2] = -np.inf
    if W > 2:
        z[:, W - 1] = np.nan                                      # a nodata border column
    return z


PATTERNS = {
    "cone": cone,
    "ramp_x": lambda H, W: np.broadcast_to(np.arange(W - 1, -1, -1, dtype=np.float32), (H, W)).copy(),
    "ramp_diag": lambda H, W: np.add.outer(np.arange(H - 1, -1, -1), np.arange(W - 1, -1, -1)).astype(np.float32),
    "spiral": lambda H, W: _trench(RO.spiral(H, W)),
    "serpentine": lambda H, W: _trench(RO.serpentine(H, W)),
    "terraces": terraces,
    "noise": noise,
    "constant": lambda H, W: np.ones((H, W), dtype=np.float32),
    "holes": holes,
    "checkerboard": lambda H, W: RO.checkerboard(H, W).astype(np.float32),
}
