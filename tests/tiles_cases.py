"""Shared by the tiled-inference suites (test_tiles_host.py, test_gpu_tiles.py): the seeded inputs of the tile-fold
comparisons, the chained fold + merge cases, and one cached host reference per case, computed once per process and left
unchanged.

FOLD    lists of 0 .. 1000 rows in TILE coordinates on a 400 x 300 frame, built row by row from a keep pattern
        (views_cases._pattern). Every view has one of the geometries of GEOM below: the whole frame, a corner tile with two
        interior sides, a tile with four interior sides, and a window that runs over the frame's right and bottom edge (no
        plan makes one; the kernel must still drop what lands off the frame after the translation). A row meant to stay
        lies inside its tile clear of the seams, exactly ON a seam limit, or hangs over a frame-side edge and is clipped; a
        row meant to go lies beyond the tile, within the margin of an interior side (from a quarter pixel inside the limit
        on), runs past an interior side, has a NaN coordinate, has an area outside the view's window, or lands off the
        frame. `reasons` records which. Coordinates, offsets, sizes and limits are multiples of 0.25 below 2^11: translation
        and mirroring are exact, so the pattern is known beforehand and is the same for a mirrored view. The table's rows are
        15 floats apart, the last two a marker; the lists are packed with gaps of 1 .. 5 rows, the first at row 3.
CHAINED soft_merge_cases.cluster_lists on a frame cut into a left and a right tile that share a strip (beside a full-frame
        view in the larger case); a view's list is the clusters in ITS coordinates -- mirrored first when the view is, then
        shifted by the tile's offset, in float32 -- so the fold lands within a rounding of the cluster again, and the
        clusters a tile's side cuts are dropped by the seam rule. The seeds were chosen so that the margins of the host
        restatements hold on the FOLDED lists (test_tiles_host.py asserts it)."""
import functools

import numpy as np

import soft_merge_cases as C
import views_cases as VC
from dana_amd import postprocess as PP

FW, FH = VC.FW, VC.FH
WINDOW = VC.WINDOW
STRIDE = 15
MARKER = 12345.0
LENGTHS = VC.LENGTHS
INF = np.inf
M = 4.25  # the seam margin of the fold cases, original-image pixels

# name -> (x_off, y_off, tw, th, lim_x1, lim_y1, lim_x2, lim_y2)
GEOM = {
    "full": (0.0, 0.0, FW, FH, -INF, -INF, INF, INF),
    "top_left": (0.0, 0.0, 220.5, 170.25, -INF, -INF, 220.5 - 1 - M, 170.25 - 1 - M),
    "bottom_right": (179.5, 129.75, 220.5, 170.25, M, M, INF, INF),
    "middle": (90.25, 60.5, 220.5, 170.25, M, M, 220.5 - 1 - M, 170.25 - 1 - M),
    "over": (300.0, 200.0, 220.5, 170.25, M, M, INF, INF),  # runs 120.5 x 70.25 pixels over the frame
}
REASONS = ("inside", "on_limit", "clipped", "beyond", "margin", "past", "nan", "area", "off_frame")

# name -> (B, V, C)
FOLD_SHAPES = {"b1v1c1": (1, 1, 1), "b1v2c1": (1, 2, 1), "b2v5c2": (2, 5, 2), "b1v10c3": (1, 10, 3)}


def _quarter(x):
    return np.round(np.asarray(x) * 4.0) / 4.0


def _rows(rng, keep, geom, window, all_nan=False):
    """float32 [n,5] in tile coordinates, descending score order, whose row k survives the fold iff keep[k]; and why"""
    n = len(keep)
    off, size, lim1, lim2 = np.asarray(geom[0:2]), np.asarray(geom[2:4]), np.asarray(geom[4:6]), np.asarray(geom[6:8])
    eff = np.minimum(size, np.asarray((FW, FH)) - off)  # the part of the tile that lies on the frame
    lo = np.where(np.isfinite(lim1), lim1, 0.0)
    hi = np.where(np.isfinite(lim2), lim2, eff - 1.0)
    span = (20, 40) if window is not None else (21, 60)  # with a window: (w + 1) * (h + 1) in [441, 1681]
    wh = _quarter(rng.uniform(span[0], span[1], (n, 2)))
    p1 = _quarter(lo + rng.uniform(0, 1, (n, 2)) * (hi - wh - lo))  # inside, clear of every seam
    p2 = p1 + wh
    reasons = ["inside"] * n
    for k in range(n):
        a = rng.randint(2)  # the axis it happens on
        if keep[k]:
            kind = rng.randint(3) if window is None else rng.randint(2)
            if kind == 1 and (np.isfinite(lim1[a]) or np.isfinite(lim2[a])):
                if np.isfinite(lim1[a]) and (rng.randint(2) or not np.isfinite(lim2[a])):
                    p1[k, a] = lim1[a]
                else:
                    p1[k, a] = lim2[a] - wh[k, a]
                reasons[k] = "on_limit"
            elif kind == 2:  # over a frame-side edge of the tile by up to 20 pixels; only views without an area window
                if not np.isfinite(lim1[a]):
                    p1[k, a] = -_quarter(rng.uniform(0.25, 20))
                    reasons[k] = "clipped"
                elif not np.isfinite(lim2[a]):
                    p1[k, a] = eff[a] - 1.0 + _quarter(rng.uniform(0.25, 20)) - wh[k, a]
                    reasons[k] = "clipped"
            p2[k, a] = p1[k, a] + wh[k, a]
            continue
        kind = 3 if all_nan else rng.randint(6)
        if kind == 4 and window is None:
            kind = 0
        if kind == 5 and eff[a] == size[a]:
            kind = 1
        if kind in (1, 2) and not (np.isfinite(lim1[a]) or np.isfinite(lim2[a])):
            kind = 0
        if kind == 0:  # beyond the tile: past its far side from a quarter pixel on, or before its near side
            if rng.randint(2):
                p1[k, a] = size[a] - 1.0 + _quarter(rng.uniform(0.25, 50))
                p2[k, a] = p1[k, a] + wh[k, a]
            else:
                p2[k, a] = -_quarter(rng.uniform(0.25, 30))
                p1[k, a] = p2[k, a] - wh[k, a]
            reasons[k] = "beyond"
        elif kind == 1:  # within the margin of an interior side, from a quarter pixel inside the limit on
            d = _quarter(rng.uniform(0.25, M))
            if np.isfinite(lim1[a]) and (rng.randint(2) or not np.isfinite(lim2[a])):
                p1[k, a] = lim1[a] - d
            else:
                p1[k, a] = lim2[a] + d - wh[k, a]
            p2[k, a] = p1[k, a] + wh[k, a]
            reasons[k] = "margin"
        elif kind == 2:  # past an interior side, into what would be the holder's padding or the neighbour's pixels
            d = _quarter(rng.uniform(0.25, 15))
            if np.isfinite(lim1[a]) and (rng.randint(2) or not np.isfinite(lim2[a])):
                p1[k, a] = -d
            else:
                p1[k, a] = size[a] - 1.0 + d - wh[k, a]
            p2[k, a] = p1[k, a] + wh[k, a]
            reasons[k] = "past"
        elif kind == 3:
            (p1, p2)[rng.randint(2)][k, a] = np.nan
            reasons[k] = "nan"
        elif kind == 4:  # too small or too large for the window
            side = _quarter(rng.uniform(5, 15) if rng.randint(2) else rng.uniform(45, 60))
            p1[k] = _quarter(lo + rng.uniform(0, 1, 2) * (hi - side - lo))
            p2[k] = p1[k] + side
            reasons[k] = "area"
        else:  # on the tile, clear of its seams, but off the frame once translated
            p1[k, a] = eff[a] + _quarter(rng.uniform(0, 40))
            p2[k, a] = p1[k, a] + wh[k, a]
            reasons[k] = "off_frame"
    score = np.sort(rng.uniform(0.05, 1.0, n))[::-1]
    return np.stack((p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1], score), 1).astype(np.float32), reasons


def _fold_spec(name):
    """-> per problem p (length, pattern), per view (geometry, flip, window)"""
    B, V, Cn = FOLD_SHAPES[name]
    if name == "b1v1c1":
        return [(1000, "first")], [("middle", 0, None)]
    if name == "b1v2c1":
        return [(256, "chunk_last"), (1000, "chunk_last")], [("top_left", 0, None), ("bottom_right", 1, None)]
    if name == "b2v5c2":
        lists = [(0, "none"), (1, "none"), (63, "other"), (64, "all"), (65, "none"), (255, "other"), (256, "none"),
                 (257, "all"), (1000, "other"), (257, "nan"), (64, "first"), (1000, "none"), (255, "random"), (1, "all"),
                 (257, "other"), (65, "random"), (63, "none"), (256, "random"), (1000, "random"), (0, "none")]
        views = [("full", 0, None), ("top_left", 0, None), ("bottom_right", 1, None), ("middle", 0, WINDOW), ("over", 1, None),
                 ("full", 1, WINDOW), ("middle", 1, None), ("over", 0, None), ("top_left", 1, WINDOW), ("bottom_right", 0, None)]
        return lists, views
    kinds = ("random", "none", "other", "all", "first", "chunk_last")
    lists = [(LENGTHS[(2 * p + 1) % len(LENGTHS)], kinds[p % len(kinds)]) for p in range(B * V * Cn)]
    geoms = ("full", "full", "top_left", "top_left", "bottom_right", "bottom_right", "middle", "middle", "over", "over")
    return lists, [(geoms[v], v % 2, WINDOW if v in (3, 6) else None) for v in range(V)]


@functools.lru_cache(maxsize=None)
def fold_inputs(name):
    """-> (lists in problem order, table float32 [B*V][STRIDE], packed float32 [rows,5] with gaps, counts int32 [P],
    offsets int32 [P+1], reasons per list)"""
    B, V, Cn = FOLD_SHAPES[name]
    spec, per_view = _fold_spec(name)
    rng = np.random.RandomState(sorted(FOLD_SHAPES).index(name) + 60)
    lists, reasons = [], []
    for p, (n, kind) in enumerate(spec):
        geom, flip, window = per_view[p // Cn]
        rows, why = _rows(rng, VC._pattern(kind, n, rng), GEOM[geom], window, all_nan=kind == "nan")
        lists.append(rows)
        reasons.append(why)
    table = np.full((B * V, STRIDE), MARKER, np.float32)
    for iv, (geom, flip, window) in enumerate(per_view):
        table[iv, :13] = (FW, FH, flip) + ((-INF, INF) if window is None else window) + GEOM[geom]
    counts = np.asarray([len(q) for q in lists], np.int32)
    offsets, at = np.zeros(len(lists) + 1, np.int32), 3
    for p, n in enumerate(counts):
        offsets[p] = at
        at += int(n) + 1 + (p * 7) % 5
    offsets[-1] = at
    packed = np.full((at, 5), 777.0, np.float32)
    for p, q in enumerate(lists):
        packed[offsets[p]:offsets[p] + len(q)] = q
    return lists, table, packed, counts, offsets, reasons


@functools.lru_cache(maxsize=None)
def fold_reference(name):
    B, V, Cn = FOLD_SHAPES[name]
    lists, table = fold_inputs(name)[:2]
    return PP.fold_tiles_numpy(lists, table, V, Cn)


# ---- fold + merge -------------------------------------------------------------------------------------------------------

# name -> (seed, B, C, rows per problem p = (i * V + v) * C + c, per view (tile, flip)); every (image, class) concatenates
# at most 80 rows. "left" / "right" are the two tiles of the frame (in the view's own, possibly mirrored, frame).
CHAINED = {
    "v2": (0, 1, 1, (40, 30), (("left", 0), ("right", 1))),
    "b2v3c2": (1, 2, 2, (20, 9, 25, 0, 14, 30, 0, 26, 31, 20, 12, 33), (("full", 0), ("left", 0), ("right", 1))),
}
CHAINED_RUNS = VC.CHAINED_RUNS
VOTE = VC.VOTE
SEAM = 8.0


@functools.lru_cache(maxsize=None)
def chained_clean(name):
    """the lists in frame coordinates, before any mirroring or shifting"""
    seed, B, Cn, counts, per_view = CHAINED[name]
    return C.cluster_lists(seed, counts)


@functools.lru_cache(maxsize=None)
def chained_inputs(name):
    """-> (lists in their views' tile coordinates, table [B*V][13], B, V, C)"""
    seed, B, Cn, counts, per_view = CHAINED[name]
    V = len(per_view)
    clean = chained_clean(name)
    fw = float(np.ceil(max(float(q[:, 2].max(initial=0)) for q in clean)) + 50.0)
    fh = float(np.ceil(max(float(q[:, 3].max(initial=0)) for q in clean)) + 50.0)
    # two tiles over the whole height: the left one ends at 0.6 fw, the right one starts at 0.4 fw (quarter pixels)
    cut_hi, cut_lo = float(_quarter(0.6 * fw)), float(_quarter(0.4 * fw))
    geom = {"full": (0.0, 0.0, fw, fh, -INF, -INF, INF, INF),
            "left": (0.0, 0.0, cut_hi, fh, -INF, -INF, cut_hi - 1.0 - SEAM, INF),
            "right": (cut_lo, 0.0, fw - cut_lo, fh, SEAM, -INF, INF, INF)}
    table = np.zeros((B * V, 13), np.float32)
    lists = []
    for p, q in enumerate(clean):
        iv = p // Cn
        tile, flip = per_view[iv % V]
        table[iv] = (fw, fh, flip, -INF, INF) + geom[tile]
        q = q.copy()
        if flip:
            wm1 = np.float32(fw) - np.float32(1.0)
            q[:, 0], q[:, 2] = wm1 - q[:, 2], wm1 - q[:, 0]
        q[:, 0] -= table[iv, 5]
        q[:, 2] -= table[iv, 5]
        q[:, 1] -= table[iv, 6]
        q[:, 3] -= table[iv, 6]
        lists.append(q)
    return lists, table, B, V, Cn


@functools.lru_cache(maxsize=None)
def folded_reference(name):
    lists, table, B, V, Cn = chained_inputs(name)
    return PP.fold_tiles_numpy(lists, table, V, Cn)


@functools.lru_cache(maxsize=None)
def chained_reference(name, method, vote):
    V = len(CHAINED[name][4])
    return PP.merge_soft_numpy(folded_reference(name)["dets"], V, C.THR, method=method, vote_thresh=VOTE if vote else None)


@functools.lru_cache(maxsize=None)
def plain_views_reference(name):
    """the same lists read as plain views (table columns 0..4 only): what the dispatch check of test_gpu_tiles.py expects"""
    lists, table, B, V, Cn = chained_inputs(name)
    return PP.fold_views_numpy(lists, table[:, :5], V, Cn)
