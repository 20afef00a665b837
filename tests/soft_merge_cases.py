"""Shared by the soft-NMS / box-voting suites (test_soft_merge_host.py, test_gpu_soft_merge.py): the seeded detection lists,
the parameter sets each of them is run with, and one cached `postprocess.merge_soft_numpy` result per (case, parameters).

Three families of cases:
  SMALL  concatenations of at most 80 rows: run under every method, with and without voting. The Gaussian comparison and
         the voting runs need the restatement's `pick` and `drop` margins >= 1e-4; the seeds below were chosen so that
         they hold (test_soft_merge_host.py asserts it on the CPU).
  LONG   lists of 255 .. 600 rows (more than two rows per thread of the 256-thread workgroup, more than one 256-row chunk
         of the voting kernel): hard and linear, and voting after hard only -- a linear run with voting would need the pick
         margin, and among 600 decaying scores two come closer than 1e-4 at some pick (about n^2 / 2 * 1e-4 = 18 expected
         near-ties); the bit-for-bit comparisons without voting need no margin.
  TIES   equal input scores, and two rows decayed to the same working score: hard and linear without voting, bit for bit."""
import functools

import numpy as np

from dana_amd import postprocess as PP

THR = 0.3
SCALES = (1.0, 0.4, 0.15)
MARGIN = 1e-4  # 10x the Gaussian tolerance at L = 80 rows (80 * 2**-23 = 9.6e-6)


def cluster_lists(seed, counts, clusters=None):
    """len(counts) float32 lists [k,5] in descending score order, scores pairwise distinct over all lists; boxes in well
    separated clusters of three nested sizes: equal sizes overlap almost completely (IoU > 0.8), different ones hardly"""
    rng = np.random.RandomState(seed)
    total = int(sum(counts))
    clusters = clusters or max(total // 12, 2)
    cols = int(np.ceil(np.sqrt(clusters)))
    score = ((rng.permutation(total) + 1.0) / (total + 1.0)).astype(np.float32)
    out, at = [], 0
    for k in counts:
        c = rng.randint(0, clusters, k)
        side = 200.0 * np.asarray(SCALES)[rng.randint(0, 3, k)]
        cx = 150.0 + 300.0 * (c % cols) + rng.uniform(-0.01, 0.01, k) * side
        cy = 150.0 + 300.0 * (c // cols) + rng.uniform(-0.01, 0.01, k) * side
        w, h = side * rng.uniform(0.98, 1.02, k), side * rng.uniform(0.98, 1.02, k)
        d = np.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score[at:at + k]), 1).astype(np.float32)
        out.append(d[np.argsort(-d[:, 4], kind="stable")])
        at += k
    return out


def scattered_lists(seed, counts):
    """the same, but boxes of random size thrown over one 400 x 400 field: every IoU between 0 and 1 occurs"""
    rng = np.random.RandomState(seed)
    total = int(sum(counts))
    score = ((rng.permutation(total) + 1.0) / (total + 1.0)).astype(np.float32)
    out, at = [], 0
    for k in counts:
        x1, y1 = rng.uniform(0, 300, k), rng.uniform(0, 300, k)
        w, h = rng.uniform(20, 160, k), rng.uniform(20, 160, k)
        d = np.stack((x1, y1, x1 + w, y1 + h, score[at:at + k]), 1).astype(np.float32)
        out.append(d[np.argsort(-d[:, 4], kind="stable")])
        at += k
    return out


def equal_score_lists():
    """ties inside a list, the same boxes with the same scores in the next group, and equal scores on disjoint boxes"""
    a = cluster_lists(17, (12,), clusters=12)[0]
    a[:, 4] = np.asarray([0.9, 0.9, 0.8, 0.8, 0.8, 0.7, 0.6, 0.6, 0.5, 0.5, 0.5, 0.5], np.float32)
    b = a.copy()
    c = a.copy()
    c[:, :4] += np.float32(5000.0)
    return [a, b, c]


def decayed_tie_lists():
    """the worked case's A, B, C, D with B and C at one score: iou(A,B) = iou(A,C) = 0.5 by symmetry, so the linear method
    decays both to exactly 0.8 * 0.5 and the lower concatenation index must be picked first. B and C sit in different
    groups, and a second list holds them the other way round."""
    A, D = [0, 0, 9, 9, .9], [20, 20, 29, 29, .6]
    B, C = [0, 0, 9, 4, .8], [0, 5, 9, 9, .8]
    f = lambda *rows: np.asarray(rows, np.float32).reshape(-1, 5)  # noqa: E731
    return [f(A, B), f(C, D), f(A, C), f(B, D)]


# name -> (lists, groups)
SMALL = {
    "edges": (cluster_lists(0, (0, 1, 2, 63, 64, 65)), 1),                # the wave edges; an empty list in front
    "empty_between": (cluster_lists(0, (5, 9, 0, 0, 30, 40)), 2),         # an all-empty list between two others
    "empty_middle_group": (cluster_lists(0, (40, 0, 30), clusters=6), 3),  # groups = 3, the middle one empty
    "scattered": (scattered_lists(0, (50, 30)), 2),                       # IoUs on both sides of every threshold
}
LONG = {
    "long": (cluster_lists(3, (255, 256, 257, 600)), 1),                  # the workgroup edges, > 2 rows per thread
    "long_groups": (cluster_lists(4, (250, 0, 350, 1, 0, 2)), 3),         # 600 rows out of three groups, beside a 3-row list
}
TIES = {
    "equal_scores": (equal_score_lists(), 3),
    "decayed_tie": (decayed_tie_lists(), 2),
}
CASES = dict(SMALL, **LONG, **TIES)

# parameter sets beside the defaults (nms_thresh THR, min_score 0.001, max_dets 0, strict >): name -> keywords
VARIANTS = {
    "plain": {},
    "ge": dict(nms_inclusive=True),
    "max1": dict(max_dets=1),
    "max7": dict(max_dets=7),          # inside every list that has more than 7 rows
    "max1000": dict(max_dets=1000),    # above every list
    "drop": dict(min_score=0.05),      # rows are dropped in the middle of the loop, after a decay
}
VOTE = 0.5


@functools.lru_cache(maxsize=None)
def reference(case, method, vote=False, variant="plain", vote_score="id"):
    """merge_soft_numpy of one case, computed once per process and shared (read-only) by the tests"""
    lists, groups = CASES[case]
    kw = dict(nms_thresh=THR, method=method, vote_thresh=VOTE if vote else None, vote_score=vote_score)
    kw.update(VARIANTS[variant])
    return PP.merge_soft_numpy(lists, groups, **kw)


def runs():
    """every (case, method, vote, variant, vote_score) the GPU file compares, in one place so that the host file can check
    the margins of exactly these"""
    out = []
    for case in SMALL:
        for method in ("hard", "linear", "gaussian"):
            out += [(case, method, False, "plain", "id"), (case, method, True, "plain", "id"), (case, method, True, "plain", "avg")]
        for variant in ("ge", "max1", "max7", "max1000", "drop"):
            for method in ("linear", "gaussian"):
                out.append((case, method, variant == "max7", variant, "id"))
    for case in LONG:
        out += [(case, "hard", False, "plain", "id"), (case, "hard", True, "plain", "id"), (case, "linear", False, "plain", "id"),
                (case, "linear", False, "max7", "id"), (case, "linear", False, "drop", "id")]
    for case in TIES:
        out += [(case, "hard", False, "plain", "id"), (case, "linear", False, "plain", "id"), (case, "linear", False, "ge", "id"),
                (case, "linear", False, "max7", "id")]
    return out


def needs_margin(method, vote):
    return method == "gaussian" or vote
