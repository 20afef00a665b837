"""Shared by the view-ensemble suites (test_views_host.py, test_gpu_views.py): the seeded inputs of the fold comparisons, the
chained fold + merge cases, and one cached host reference per case, computed once per process and left unchanged.

FOLD    lists of 0 .. 1000 rows on a 400 x 300 frame, built row by row from a keep pattern: a row meant to stay lies on the
        frame (some hang over an edge and are clipped), a row meant to go lies beyond the right or above the top edge, has a
        NaN coordinate, or -- in views with an area window -- an area outside the window. Coordinates are quarter pixels,
        so mirroring them beforehand is exact and the pattern is the same whether the view is mirrored or not. The lists
        are packed with gaps of 1 .. 5 rows between them, the first at row 3.
CHAINED soft_merge_cases.cluster_lists on a frame that holds every box, half of the views mirrored beforehand (in float32:
        the fold's un-mirroring lands within a rounding of the cluster again). The seeds were chosen so that the margins of
        the host restatements hold on the FOLDED lists (test_views_host.py asserts it)."""
import functools

import numpy as np

import soft_merge_cases as C
from dana_amd import postprocess as PP

FW, FH = 400.0, 300.0
WINDOW = (400.0, 1700.0)
STRIDE = 7  # the fold tests' table rows are 7 floats apart, two of them unused
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)

# name -> (B, V, C)
FOLD_SHAPES = {"b1v1c1": (1, 1, 1), "b1v2c1": (1, 2, 1), "b2v3c2": (2, 3, 2), "b1v6c3": (1, 6, 3)}


def _quarter(x):
    return np.round(np.asarray(x) * 4.0) / 4.0


def _pattern(kind, n, rng):
    keep = np.zeros(n, bool)
    if kind == "none":
        keep[:] = True
    elif kind == "other":
        keep[::2] = True
    elif kind == "first":
        keep[:1] = True
    elif kind == "chunk_last":  # only the last row of every full 256-row chunk
        keep[255::256] = True
    elif kind == "random":
        keep = rng.uniform(size=n) < 0.5
    elif kind not in ("all", "nan"):
        raise KeyError(kind)
    return keep


def _rows(rng, keep, flip, window, all_nan=False):
    """float32 [n,5] in descending score order whose row k survives the fold iff keep[k]"""
    n = len(keep)
    wm1, hm1 = FW - 1.0, FH - 1.0
    if window is None:  # on the frame, up to 20 pixels over its edges
        w, h = _quarter(rng.uniform(21, 60, n)), _quarter(rng.uniform(21, 60, n))
        x1, y1 = _quarter(rng.uniform(-20, wm1 - 30, n)), _quarter(rng.uniform(-20, hm1 - 30, n))
        x1[:2], y1[:2] = (wm1, -20.0)[:n], (0.0, hm1)[:n]  # x1 == wm1 and y1 == hm1 exactly
    else:  # inside the frame with an area inside the window: (w + 1) * (h + 1) in [441, 1681]
        w, h = _quarter(rng.uniform(20, 40, n)), _quarter(rng.uniform(20, 40, n))
        x1, y1 = _quarter(rng.uniform(0, wm1 - 41, n)), _quarter(rng.uniform(0, hm1 - 41, n))
    x2, y2 = x1 + w, y1 + h
    kinds = rng.randint(0, 4 if window is not None else 3, n)
    for k in np.nonzero(~keep)[0]:
        if all_nan or kinds[k] == 2:
            (x1, y1, x2, y2)[rng.randint(0, 4)][k] = np.nan
        elif kinds[k] == 0:  # beyond the right edge, from one quarter pixel on
            x1[k] = wm1 + _quarter(rng.uniform(0.25, 50))
            x2[k] = x1[k] + w[k]
        elif kinds[k] == 1:  # above the top edge
            y2[k] = -_quarter(rng.uniform(0.25, 30))
            y1[k] = y2[k] - h[k]
        else:  # too small or too large for the window
            side = _quarter(rng.uniform(5, 15) if rng.randint(2) else rng.uniform(45, 60))
            x2[k], y2[k] = x1[k] + side, y1[k] + side
    if flip:
        x1, x2 = wm1 - x2, wm1 - x1  # exact on quarter pixels
    score = np.sort(rng.uniform(0.05, 1.0, n))[::-1]
    return np.stack((x1, y1, x2, y2, score), 1).astype(np.float32)


def _fold_spec(name):
    """-> per problem p (length, pattern), per view (flip, window)"""
    B, V, Cn = FOLD_SHAPES[name]
    if name == "b1v1c1":
        return [(1000, "first")], [(0, None)]
    if name == "b1v2c1":
        return [(256, "chunk_last"), (1000, "chunk_last")], [(0, None), (1, None)]
    if name == "b2v3c2":
        lists = [(0, "none"), (1, "none"), (63, "other"), (64, "all"), (65, "none"), (255, "other"),
                 (256, "none"), (257, "all"), (1000, "other"), (257, "nan"), (64, "first"), (1000, "none")]
        return lists, [(0, None), (1, None), (0, WINDOW), (1, WINDOW), (1, None), (0, None)]
    kinds = ("random", "none", "other", "all", "first", "chunk_last")
    lists = [(LENGTHS[(2 * p + 1) % len(LENGTHS)], kinds[p % len(kinds)]) for p in range(B * V * Cn)]
    return lists, [(v % 2, WINDOW if v in (2, 3) else None) for v in range(V)]


@functools.lru_cache(maxsize=None)
def fold_inputs(name):
    """-> (lists in problem order, table float32 [B*V][STRIDE], packed float32 [rows,5] with gaps, counts int32 [P],
    offsets int32 [P+1])"""
    B, V, Cn = FOLD_SHAPES[name]
    spec, per_view = _fold_spec(name)
    rng = np.random.RandomState(sorted(FOLD_SHAPES).index(name) + 40)
    lists = []
    for p, (n, kind) in enumerate(spec):
        flip, window = per_view[p // Cn]
        lists.append(_rows(rng, _pattern(kind, n, rng), flip, window, all_nan=kind == "nan"))
    table = np.full((B * V, STRIDE), 12345.0, np.float32)
    for iv, (flip, window) in enumerate(per_view):
        table[iv, :5] = (FW, FH, flip) + ((-np.inf, np.inf) if window is None else window)
    counts = np.asarray([len(q) for q in lists], np.int32)
    offsets, at = np.zeros(len(lists) + 1, np.int32), 3
    for p, n in enumerate(counts):
        offsets[p] = at
        at += int(n) + 1 + (p * 7) % 5
    offsets[-1] = at
    packed = np.full((at, 5), 777.0, np.float32)
    for p, q in enumerate(lists):
        packed[offsets[p]:offsets[p] + len(q)] = q
    return lists, table, packed, counts, offsets


@functools.lru_cache(maxsize=None)
def fold_reference(name):
    B, V, Cn = FOLD_SHAPES[name]
    lists, table = fold_inputs(name)[:2]
    return PP.fold_views_numpy(lists, table, V, Cn)


# ---- fold + merge -------------------------------------------------------------------------------------------------------

# name -> (seed, B, V, C, rows per problem p = (i * V + v) * C + c); every (image, class) concatenates at most 80 rows
CHAINED = {
    "v2": (0, 1, 2, 1, (40, 30)),
    "b2v3c2": (1, 2, 3, 2, (20, 9, 25, 0, 14, 30, 0, 26, 31, 20, 12, 33)),
}
CHAINED_RUNS = [(m, v) for m in ("hard", "linear", "gaussian") for v in (False, True)]
VOTE = 0.8


@functools.lru_cache(maxsize=None)
def chained_clean(name):
    """the lists before any mirroring"""
    seed, B, V, Cn, counts = CHAINED[name]
    return C.cluster_lists(seed, counts)


@functools.lru_cache(maxsize=None)
def chained_inputs(name):
    """-> (lists with the odd views mirrored, table [B*V][5], B, V, C)"""
    seed, B, V, Cn, counts = CHAINED[name]
    clean = chained_clean(name)
    fw = np.float32(np.ceil(max(float(q[:, 2].max(initial=0)) for q in clean)) + 50.0)
    fh = np.float32(np.ceil(max(float(q[:, 3].max(initial=0)) for q in clean)) + 50.0)
    table = np.zeros((B * V, 5), np.float32)
    lists = []
    for p, q in enumerate(clean):
        iv = p // Cn
        flip = (iv % V) % 2
        table[iv] = (fw, fh, flip, -np.inf, np.inf)
        q = q.copy()
        if flip:
            wm1 = fw - np.float32(1.0)
            q[:, 0], q[:, 2] = wm1 - q[:, 2], wm1 - q[:, 0]
        lists.append(q)
    return lists, table, B, V, Cn


@functools.lru_cache(maxsize=None)
def folded_reference(name):
    lists, table, B, V, Cn = chained_inputs(name)
    return PP.fold_views_numpy(lists, table, V, Cn)


@functools.lru_cache(maxsize=None)
def chained_reference(name, method, vote):
    V = CHAINED[name][2]
    return PP.merge_soft_numpy(folded_reference(name)["dets"], V, C.THR, method=method, vote_thresh=VOTE if vote else None)
