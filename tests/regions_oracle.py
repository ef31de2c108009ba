"""Plain numpy oracle of floodgan.regions: labelling, sieve and region table, written from the semantics (no device,
no scipy).

Mask: a boolean [H, W] array (flood = True).  `connectivity` (8 or 4) is that of the flood class; the dry class takes
the complementary one.  A member pixel's label is the index y * W + x of its component's first pixel in row-major
order, a non-member's -1.

The labelling is a two-pass union-find over the rows' runs: a run is united with the runs of the previous row it
touches (overlapping columns; at 8 also the diagonal neighbours), always under the smaller run number.  Runs are
numbered in row-major order of their first pixels, so the smallest run of a set starts at the set's first pixel."""
import numpy as np

COLUMNS = ("label", "area", "y0", "x0", "y1", "x1", "sum_y", "sum_x")


def _runs(row):
    d = np.diff(np.concatenate(([0], row.astype(np.int8), [0])))
    return np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()         # [start, end)


def label(mask, connectivity=8):
    """int32 [H, W] canonical labels of the True pixels of mask at the given connectivity"""
    assert connectivity in (4, 8)
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    reach = 1 if connectivity == 8 else 0
    parent, runs = [], []

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    prev = []
    for y in range(H):
        cur = []
        j = 0
        for s, e in zip(*_runs(mask[y])):
            rid = len(runs)
            runs.append((y, s, e))
            parent.append(rid)
            cur.append(rid)
            # previous-row runs [ps, pe) that touch [s, e): ps < e + reach and pe > s - reach
            while j < len(prev) and runs[prev[j]][2] <= s - reach:
                j += 1
            k = j
            while k < len(prev) and runs[prev[k]][1] < e + reach:
                a, b = find(rid), find(prev[k])
                if a != b:
                    parent[max(a, b)] = min(a, b)
                k += 1
        prev = cur
    out = np.full((H, W), -1, dtype=np.int32)
    for rid, (y, s, e) in enumerate(runs):
        ry, rs, _ = runs[find(rid)]
        out[y, s:e] = ry * W + rs
    return out


def label_class(mask, target=True, connectivity=8):
    """the labels of the flood class (target) or of the dry class, which takes the complementary connectivity"""
    mask = np.asarray(mask, dtype=bool)
    return label(mask, connectivity) if target else label(~mask, 12 - connectivity)


def sieve(mask, min_region=1, min_hole=0, connectivity=8):
    """(final mask, removed, filled): flood components below min_region removed, then the dry components below
    min_hole that hold no pixel of the outer rows or columns filled"""
    m = np.array(mask, dtype=bool)
    removed = filled = 0
    if min_region > 1:
        lab = label(m, connectivity)
        ids, counts = np.unique(lab[lab >= 0], return_counts=True)
        small = ids[counts < min_region]
        m[np.isin(lab, small)] = False
        removed = len(small)
    if min_hole > 0:
        lab = label(~m, 12 - connectivity)
        ids, counts = np.unique(lab[lab >= 0], return_counts=True)
        edge = np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])
        holes = ids[(counts < min_hole) & ~np.isin(ids, edge)]
        m[np.isin(lab, holes)] = True
        filled = len(holes)
    return m, removed, filled


def table(labels):
    """{column: int64 [R]} of a labels plane, rows in ascending label order"""
    ys, xs = np.nonzero(labels >= 0)
    ids, inv = np.unique(labels[ys, xs], return_inverse=True)
    R = len(ids)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    y0, x0 = np.full(R, labels.shape[0], np.int64), np.full(R, labels.shape[1], np.int64)
    y1, x1 = np.full(R, -1, np.int64), np.full(R, -1, np.int64)
    np.minimum.at(y0, inv, ys)
    np.minimum.at(x0, inv, xs)
    np.maximum.at(y1, inv, ys)
    np.maximum.at(x1, inv, xs)
    return {"label": ids.astype(np.int64), "area": np.bincount(inv, minlength=R).astype(np.int64),
            "y0": y0, "x0": x0, "y1": y1, "x1": x1,
            "sum_y": np.bincount(inv, weights=ys, minlength=R).astype(np.int64),
            "sum_x": np.bincount(inv, weights=xs, minlength=R).astype(np.int64)}


def flood_regions(mask, min_region=1, min_hole=0, connectivity=8):
    """the oracle of floodgan.regions.flood_regions on a boolean mask"""
    m, removed, filled = sieve(mask, min_region, min_hole, connectivity)
    lab = label(m, connectivity)
    tab = table(lab)
    area = tab["area"].astype(np.float64)
    return {"mask": m, "labels": lab, "count": len(tab["label"]), "table": tab,
            "centroids": np.stack([tab["sum_y"] / area, tab["sum_x"] / area], axis=1),
            "removed": removed, "filled": filled, "flood_fraction": int(m.sum()) / m.size}


# ---- the test patterns (boolean [H, W])

def checkerboard(H, W):
    return (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0


def spiral(H, W):
    """a one-pixel-wide rectangular spiral from the top-left corner inward, one dry pixel between its turns: one
    component at either connectivity, with the longest chain the scene allows.  The walk goes straight while the
    next pixel is inside the scene and the one after it is not flooded yet, else turns right; it ends when it can
    do neither."""
    m = np.zeros((H, W), dtype=bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    turned = False
    while True:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        free = 0 <= ny < H and 0 <= nx < W and not m[ny, nx]
        if free and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
            y, x = ny, nx
            m[y, x] = True
            turned = False
        elif turned:
            return m
        else:
            dy, dx = dx, -dy
            turned = True


def serpentine(H, W):
    """every other row flooded, consecutive flooded rows joined at alternate ends"""
    m = np.zeros((H, W), dtype=bool)
    m[0::2] = True
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def stripes(H, W, vertical):
    m = np.zeros((H, W), dtype=bool)
    if vertical:
        m[:, 0::2] = True
    else:
        m[0::2] = True
    return m


def frame_island(H, W):
    """the outer frame, and an island in the middle of the lake it encloses"""
    m = np.zeros((H, W), dtype=bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    if H >= 5 and W >= 5:
        m[H // 2 - (H // 8):H // 2 + (H // 8) + 1, W // 2 - (W // 8):W // 2 + (W // 8) + 1] = True
    return m


def bernoulli(H, W, p, seed=0):
    return np.random.default_rng(seed + 1000 * H + W).random((H, W)) < p


PATTERNS = {
    "dry": lambda H, W: np.zeros((H, W), dtype=bool),
    "flood": lambda H, W: np.ones((H, W), dtype=bool),
    "checkerboard": checkerboard,
    "spiral": spiral,
    "serpentine": serpentine,
    "vstripes": lambda H, W: stripes(H, W, True),
    "hstripes": lambda H, W: stripes(H, W, False),
    "frame_island": frame_island,
    "bernoulli_0.3": lambda H, W: bernoulli(H, W, 0.3, 3),
    "bernoulli_0.5": lambda H, W: bernoulli(H, W, 0.5, 5),
    "bernoulli_0.593": lambda H, W: bernoulli(H, W, 0.593, 593),
    "bernoulli_0.7": lambda H, W: bernoulli(H, W, 0.7, 7),
}
