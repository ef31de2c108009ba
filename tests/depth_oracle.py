"""Plain numpy oracle of floodgan.depth: the nearest-seed transform, shore, depth, fixed-point totals and the per-region
depth table, written from the definitions (no device, no scipy).

Seeds: a boolean [H, W] array.  nearest[p] = the linear index y' W + x' of the seed at the minimum squared Euclidean
distance from p, and among the seeds at that distance the one with the SMALLEST linear index; dist2[p] that distance;
both -1 everywhere when there is no seed.

  nearest_seed_brute      every pixel against every seed, the seeds listed in ascending index order: the first minimum
                          of the list is the tie rule, written out
  nearest_seed_separable  exact, for the larger shapes: per column the nearest seed row (ties to the smaller row), then
                          per row the minimum over the columns of the pair (dist2, index) in lexicographic order.  A
                          seed at the global minimum distance is at its column's minimum distance, within a column the
                          smaller row wins, so the minimum over the columns' candidates is the global one.
  shore, depth, quanta, depth_table, flood_depth   the rest of the product, all depth arithmetic in np.float32
"""
import numpy as np

Q = 1024.0
CAP = np.float32(1048576.0)


def nearest_seed_brute(seeds, chunk=256):
    seeds = np.asarray(seeds, dtype=bool)
    H, W = seeds.shape
    near = np.full(H * W, -1, dtype=np.int32)
    dist2 = np.full(H * W, -1, dtype=np.int32)
    idx = np.flatnonzero(seeds.ravel())                      # ascending linear index
    if len(idx) == 0:
        return near.reshape(H, W), dist2.reshape(H, W)
    sy, sx = (idx // W).astype(np.int32), (idx % W).astype(np.int32)
    for p0 in range(0, H * W, chunk):
        p = np.arange(p0, min(p0 + chunk, H * W), dtype=np.int32)
        d = (p[:, None] // W - sy[None, :]) ** 2 + (p[:, None] % W - sx[None, :]) ** 2
        m = d.min(axis=1)
        # the tie rule: of the seeds at the minimum, the first of the ascending list
        first = (d == m[:, None]).argmax(axis=1)
        near[p] = idx[first]
        dist2[p] = m
    return near.reshape(H, W), dist2.reshape(H, W)


def nearest_seed_separable(seeds):
    seeds = np.asarray(seeds, dtype=bool)
    H, W = seeds.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    big = 4 * (H + W)
    up = np.maximum.accumulate(np.where(seeds, rows, -big), axis=0)                    # last seed row <= y
    dn = np.minimum.accumulate(np.where(seeds, rows, big)[::-1], axis=0)[::-1]         # first seed row >= y
    col = np.where(rows - up <= dn - rows, up, dn)                                      # ties to the smaller row
    has = seeds.any(axis=0)                                                             # per column
    near = np.full((H, W), -1, dtype=np.int32)
    dist2 = np.full((H, W), -1, dtype=np.int32)
    if not has.any():
        return near, dist2
    xs = np.flatnonzero(has).astype(np.int64)
    x = np.arange(W, dtype=np.int64)
    dx2 = (x[:, None] - xs[None, :]) ** 2
    for y in range(H):
        r = col[y, xs]
        d = dx2 + ((y - r) ** 2)[None, :]
        key = d * (1 << 31) + (r * W + xs)[None, :]                                      # (dist2, index), lexicographic
        k = key.min(axis=1)
        near[y] = k % (1 << 31)
        dist2[y] = k >> 31
    return near, dist2


def shore(mask):
    """flood pixels with at least one dry 4-neighbour inside the scene"""
    m = np.asarray(mask, dtype=bool)
    dry = ~m
    s = np.zeros_like(m)
    s[1:] |= dry[:-1]
    s[:-1] |= dry[1:]
    s[:, 1:] |= dry[:, :-1]
    s[:, :-1] |= dry[:, 1:]
    return s & m


def depth(mask, elevation, nearest):
    """fp32 [H, W]: elevation[nearest] - elevation where that is > 0 on the flood pixels with a nearest shore, else 0"""
    m = np.asarray(mask, dtype=bool)
    e = np.asarray(elevation, dtype=np.float32)
    out = np.zeros(m.shape, dtype=np.float32)
    ok = m & (nearest >= 0)
    with np.errstate(invalid="ignore"):
        d = e.ravel()[np.where(ok, nearest, 0)] - e
        assert d.dtype == np.float32
        out[ok & (d > 0)] = d[ok & (d > 0)]
    return out


def quanta(d):
    d = np.asarray(d, dtype=np.float32)
    scaled = np.fmin(d, CAP) * np.float32(Q)
    assert scaled.dtype == np.float32
    return np.rint(scaled).astype(np.int64)


def depth_table(labels, d):
    """{wet_area, depth_sum_q, depth_max_q}: int64 [R], rows in ascending label order (every label of the plane)"""
    q = quanta(d)
    ids = np.unique(labels[labels >= 0])
    wet, tot, top = (np.zeros(len(ids), dtype=np.int64) for _ in range(3))
    for j, lab in enumerate(ids):
        v = q[(labels == lab) & (q > 0)]
        wet[j], tot[j], top[j] = len(v), v.sum(), v.max() if len(v) else 0
    return {"wet_area": wet, "depth_sum_q": tot, "depth_max_q": top}


def flood_depth(mask, elevation, labels=None, area=None, pixel_area=1.0):
    """the oracle of floodgan.depth.flood_depth on a boolean mask; labels / area: the regions' labels plane and the
    region table's area column"""
    m = np.asarray(mask, dtype=bool)
    s = shore(m)
    near, _ = nearest_seed_separable(s)
    d = depth(m, elevation, near)
    q = quanta(d)
    wet = q[q > 0]
    total = float(wet.sum()) / Q
    flooded = int(m.sum())
    res = {"depth": d, "nearest_shore": near, "shore_count": int(s.sum()), "wet_area": len(wet),
           "max_depth": float(wet.max() if len(wet) else 0) / Q, "mean_depth": total / flooded if flooded else 0.0,
           "volume": total * float(pixel_area)}
    if labels is not None:
        tab = depth_table(labels, d)
        tot = tab["depth_sum_q"].astype(np.float64) / Q
        tab["mean_depth"] = tot / np.asarray(area, dtype=np.float64)
        tab["max_depth"] = tab["depth_max_q"].astype(np.float64) / Q
        tab["volume"] = tot * float(pixel_area)
        res["table"] = tab
    return res
