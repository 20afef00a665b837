"""Cases for proposal recall (dana_amd/evaluate.py: `proposal_recall_numpy`, `ProposalRecallEvaluator`), shared by
test_proposal_recall_host.py and test_gpu_proposal_recall.py: hand-worked cases with their answers written out, seeded case
makers, and `recall_by_sorted_sweep`, a second restatement of the matching that shares no code with the first.

A case is dict(args=..., expect=...): `args` are the keyword arguments of `proposal_recall_numpy`; `expect` holds the
hand-worked ov / match [L,A,n_pairs] and the non-zero entries of hits {(role, t, l, a, k): n} and npos {(role, a, k): n}."""
import numpy as np


def _f32(rows):
    return np.asarray(rows, np.float32).reshape(-1, 4)


def _case(boxes, problems, gt, n_cls, expect=None, **kw):
    """problems: [(image, class, count)] over `boxes` packed in that order; gt: [(image, class, box)]"""
    counts = np.asarray([p[2] for p in problems], np.int64)
    args = dict(boxes=_f32(boxes), prob_img=np.asarray([p[0] for p in problems], np.int64),
                prob_cls=np.asarray([p[1] for p in problems], np.int64), counts=counts,
                offsets=np.cumsum(counts) - counts, gt_box=_f32([g[2] for g in gt]),
                gt_img=np.asarray([g[0] for g in gt], np.int64), gt_cls=np.asarray([g[1] for g in gt], np.int64),
                n_cls=n_cls, iou_thrs=(0.5,), limits=(0,), area_rng=["all"], gt_area=None, others=False)
    args.update(kw)
    return dict(args=args, expect=expect)


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------
# Boxes (0,0,9,h-1) are 10 wide and h high under the `+ 1.` convention: the IoU of two of them is min(h) / max(h).
S10, S12, S15, S20 = (0, 0, 9, 9), (0, 0, 9, 11), (0, 0, 9, 14), (0, 0, 9, 19)


def hand_cases():
    c = {}
    # P0 = S10, P1 = S15; G0 = S10, G1 = S12. IoU: G0 1 and 2/3, G1 5/6 and 4/5. G0 takes P0 (1); G1 is left with P1 (4/5),
    # although P0 covers it better: recall at 0.82 is 1/2 (a per-object maximum would say 2/2).
    c["shared_best"] = _case([S10, S15], [(0, 0, 2)], [(0, 0, S10), (0, 0, S12)], 1, iou_thrs=(0.5, 0.82), expect=dict(
        ov=[[[1.0, 0.8]]], match=[[[0, 1]]], hits={(0, 0, 0, 0, 0): 2, (0, 1, 0, 0, 0): 1}, npos={(0, 0, 0): 2}))
    # two identical objects; row 0 covers them at 1/2, row 1 at 1: the lower position gets row 1
    c["tie_between_objects"] = _case([S20, S10], [(0, 0, 2)], [(0, 0, S10), (0, 0, S10)], 1, iou_thrs=(0.5, 0.75), expect=dict(
        ov=[[[1.0, 0.5]]], match=[[[1, 0]]], hits={(0, 0, 0, 0, 0): 2, (0, 1, 0, 0, 0): 1}, npos={(0, 0, 0): 2}))
    # rows 1 and 2 are the same box: the lower row is the match
    c["duplicate_candidates"] = _case([S20, S10, S10], [(0, 0, 3)], [(0, 0, S10)], 1, expect=dict(
        ov=[[[1.0]]], match=[[[1]]], hits={(0, 0, 0, 0, 0): 1}, npos={(0, 0, 0): 1}))
    # three objects, two candidates: G0 = P0 and G1 = P1 at IoU 1 (G0 first: the lower position of equals); G2 = S15
    # overlaps both but nothing is left for it: IoU 0, no match
    c["candidates_run_out"] = _case([S10, S20], [(0, 0, 2)], [(0, 0, S10), (0, 0, S20), (0, 0, S15)], 1, expect=dict(
        ov=[[[1.0, 1.0, 0.0]]], match=[[[0, 1, -1]]], hits={(0, 0, 0, 0, 0): 2}, npos={(0, 0, 0): 3}))
    # rows: S20 (1/2), S10 (1), S12 (5/6) against G = S10, under budgets of 1, 2 and the whole list
    c["limit"] = _case([S20, S10, S12], [(0, 0, 3)], [(0, 0, S10)], 1, iou_thrs=(0.5, 0.75), limits=(1, 2, 0), expect=dict(
        ov=[[[0.5]], [[1.0]], [[1.0]]], match=[[[0]], [[1]], [[1]]],
        hits={(0, 0, 0, 0, 0): 1, (0, 0, 1, 0, 0): 1, (0, 0, 2, 0, 0): 1, (0, 1, 1, 0, 0): 1, (0, 1, 2, 0, 0): 1},
        npos={(0, 0, 0): 1}))
    # areas 32*32 = 1024 (on the bound small / medium shares), 33*32 = 1056, 96*96 = 9216 (on the bound medium / large
    # shares), 97*96 = 9312; each object has its own copy as a candidate. Both ends of a range are inclusive.
    O = [(0, 0, 31, 31), (40, 0, 72, 31), (0, 100, 95, 195), (100, 100, 196, 195)]
    gt = [(0, 0, o) for o in O]
    c["area_of_the_box"] = _case(O, [(0, 0, 4)], gt, 1, area_rng=["small", "medium", "large"], expect=dict(
        ov=[[[1., -1., -1., -1.], [1., 1., 1., -1.], [-1., -1., 1., 1.]]],
        match=[[[0, -1, -1, -1], [0, 1, 2, -1], [-1, -1, 2, 3]]],
        hits={(0, 0, 0, 0, 0): 1, (0, 0, 0, 1, 0): 3, (0, 0, 0, 2, 0): 2},
        npos={(0, 0, 0): 1, (0, 1, 0): 3, (0, 2, 0): 2}))
    # the same boxes with areas given: 1025 (medium only), 1024 (small and medium), 9216.5 (large only), 100 (small)
    c["area_given"] = _case(O, [(0, 0, 4)], gt, 1, area_rng=["small", "medium", "large"],
                            gt_area=np.asarray([1025., 1024., 9216.5, 100.]), expect=dict(
        ov=[[[-1., 1., -1., 1.], [1., 1., -1., -1.], [-1., -1., 1., -1.]]],
        match=[[[-1, 1, -1, 3], [0, 1, -1, -1], [-1, -1, 2, -1]]],
        hits={(0, 0, 0, 0, 0): 2, (0, 0, 0, 1, 0): 2, (0, 0, 0, 2, 0): 1},
        npos={(0, 0, 0): 2, (0, 1, 0): 2, (0, 2, 0): 1}))
    # One image, objects g0..g3 of classes 1, 0, 2, 1 at x = 0, 20, 40, 60 (disjoint), lists for class 0 and class 1.
    # (image, class) order: g1 | g0 g3 | g2. Units: target A (class 0): g1; target B (class 1): g0 g3; other A: g0 g3 g2
    # (second range only); other B: g1 and g2 (one object in each range). Pairs in that order: 1 + 2 + 3 + 2.
    #   list A = copies of g1, g0: target A: g1 <- row 0 (1). other A: g0 <- row 1 (1); g3 and g2 tie at IoU 0 on row 0,
    #     g3 (lower position) takes it -- an IoU of 0 is still a match -- and g2 is left without a candidate.
    #   list B = copies of g0, g2: target B: g0 <- row 0 (1), g3 <- row 1 (IoU 0). other B: g2 <- row 1 (1), g1 <- row 0 (0).
    D = [(20 * i, 0, 20 * i + 9, 9) for i in range(4)]
    c["other_units"] = _case([D[1], D[0], D[0], D[2]], [(0, 0, 2), (0, 1, 2)],
                             [(0, 1, D[0]), (0, 0, D[1]), (0, 2, D[2]), (0, 1, D[3])], 3, others=True, expect=dict(
        ov=[[[1., 1., 0., 1., 0., 0., 0., 1.]]], match=[[[0, 0, 1, 1, 0, -1, 0, 1]]],
        pair_gt=[1, 0, 3, 0, 3, 2, 1, 2],
        hits={(0, 0, 0, 0, 0): 1, (0, 0, 0, 0, 1): 1, (1, 0, 0, 0, 0): 1, (1, 0, 0, 0, 1): 1},
        npos={(0, 0, 0): 1, (0, 0, 1): 2, (1, 0, 0): 3, (1, 0, 1): 2}, recalls={(0, 0, 0, 0): 2. / 3., (1, 0, 0, 0): 2. / 5.}))
    # the same list twice (two shot views of one class): two trials
    c["duplicated_problem"] = _case([S10, S10], [(0, 0, 1), (0, 0, 1)], [(0, 0, S10)], 1, expect=dict(
        ov=[[[1.0, 1.0]]], match=[[[0, 0]]], hits={(0, 0, 0, 0, 0): 2}, npos={(0, 0, 0): 2}))
    # the class-1 object has no list of its image: it does not count
    c["no_problem_for_class"] = _case([S10], [(0, 0, 1)], [(0, 1, S12), (0, 0, S10), (1, 0, S10)], 2, expect=dict(
        ov=[[[1.0]]], match=[[[0]]], pair_gt=[1], hits={(0, 0, 0, 0, 0): 1}, npos={(0, 0, 0): 1}))
    # an empty list: the small object is missed, the large one is outside the range
    c["empty_list"] = _case([], [(0, 0, 0)], [(0, 0, S10), (0, 0, (0, 0, 99, 99))], 1, area_rng=["small"], expect=dict(
        ov=[[[0.0, -1.0]]], match=[[[-1, -1]]], hits={}, npos={(0, 0, 0): 1}))
    return c


def dense(sparse, shape):
    out = np.zeros(shape, np.int64)
    for k, v in sparse.items():
        out[k] = v
    return out


# ---- the second restatement ---------------------------------------------------------------------------------------------------
AREAS = {"all": (0., 1e10), "small": (0., 1024.), "medium": (1024., 9216.), "large": (9216., 1e10), "96-128": (9216., 16384.),
         "128-256": (16384., 65536.), "256-512": (65536., 262144.), "512-inf": (262144., 1e10)}  # squares of the names' ends


def _iou(b, g):
    """two boxes as Python floats (IEEE doubles): the operations of evaluate._iou_matrix in its order"""
    ixmin, iymin = max(g[0], b[0]), max(g[1], b[1])
    ixmax, iymax = min(g[2], b[2]), min(g[3], b[3])
    iw, ih = max(ixmax - ixmin + 1., 0.), max(iymax - iymin + 1., 0.)
    inters = iw * ih
    uni = ((b[2] - b[0] + 1.) * (b[3] - b[1] + 1.) + (g[2] - g[0] + 1.) * (g[3] - g[1] + 1.) - inters)
    return inters / uni


def recall_by_sorted_sweep(boxes, prob_img, prob_cls, counts, offsets, gt_box, gt_img, gt_cls, n_cls, iou_thrs=None,
                           limits=(0,), area_rng=None, gt_area=None, others=False):
    """Greedy one-to-one matching as a sweep: every (IoU, object, candidate) entry of a unit, sorted by (IoU descending,
    object ascending, candidate ascending); an entry is taken when both of its sides are free. -> dict(ov, match, hits,
    npos, pair_gt), laid out as `proposal_recall_numpy` lays them out. `area_rng`: None (all of AREAS), names, or (low, high) rows."""
    thr = [float(t) for t in (np.arange(0.5, 0.96, 0.05) if iou_thrs is None else iou_thrs)]
    names = list(AREAS) if area_rng is None else area_rng
    rng = np.asarray([AREAS[x] if isinstance(x, str) else x for x in names], np.float64).reshape(-1, 2)
    b = [[float(v) for v in row] for row in np.asarray(boxes, np.float32).reshape(-1, 4)]
    g = [[float(v) for v in row] for row in np.asarray(gt_box, np.float32).reshape(-1, 4)]
    area = ([(r[2] - r[0] + 1.) * (r[3] - r[1] + 1.) for r in g] if gt_area is None else [float(x) for x in gt_area])
    P = len(counts)
    by_image = {}
    for j in sorted(range(len(g)), key=lambda j: (int(gt_img[j]), int(gt_cls[j]), j)):
        by_image.setdefault(int(gt_img[j]), []).append(j)
    units = []  # (problem, role, class, ground-truth rows)
    for role in ((0, 1) if others else (0,)):
        for p in range(P):
            c = int(prob_cls[p])
            rows = [j for j in by_image.get(int(prob_img[p]), []) if (int(gt_cls[j]) == c) == (role == 0)]
            units.append((p, role, c, rows))
    pair_gt = [j for u in units for j in u[3]]
    n_pairs, T, L, A = len(pair_gt), len(thr), len(limits), rng.shape[0]
    ov = np.full((L, A, n_pairs), -1.)
    match = np.full((L, A, n_pairs), -1, np.int64)
    hits = np.zeros((2, T, L, A, n_cls), np.int64)
    npos = np.zeros((2, A, n_cls), np.int64)
    first = 0
    for p, role, c, rows in units:
        lst = b[int(offsets[p]):int(offsets[p]) + int(counts[p])]
        for li, lim in enumerate(limits):
            cand = lst if lim <= 0 else lst[:int(lim)]
            for a in range(A):
                objs = [(q, j) for q, j in enumerate(rows) if rng[a, 0] <= area[j] <= rng[a, 1]]
                entries = sorted((-_iou(cand[i], g[j]), q, i) for q, j in objs for i in range(len(cand)))
                got, used = {}, set()
                for neg, q, i in entries:
                    if q not in got and i not in used:
                        got[q] = (-neg, i)
                        used.add(i)
                for q, j in objs:
                    v, i = got.get(q, (0., -1))
                    ov[li, a, first + q], match[li, a, first + q] = v, i
                    npos[role, a, c] += li == 0
                    for t in range(T):
                        hits[role, t, li, a, c] += v >= thr[t]
        first += len(rows)
    return dict(ov=ov, match=match, hits=hits, npos=npos, pair_gt=np.asarray(pair_gt, np.int64))


# ---- seeded cases ---------------------------------------------------------------------------------------------------------------

def _boxes(rs, n, extent, lo=6., hi=0.5):
    x1, y1 = rs.uniform(0, extent, n), rs.uniform(0, extent, n)
    w, h = rs.uniform(lo, extent * hi, n), rs.uniform(lo, extent * hi, n)
    return np.stack((x1, y1, x1 + w, y1 + h), 1)


def seeded_case(seed, lists, n_cls=1, extent=220., quantum=None, with_area=False, **kw):
    """lists: [(candidates, objects)] -- one image each. The image's objects get random classes below n_cls (the first one
    class 0); every class gets its own list of `candidates` rows, half of them jittered copies of the image's objects.
    quantum: coordinates are rounded to its multiples, so that equal IoUs occur."""
    rs = np.random.RandomState(seed)
    boxes, problems, gt = [], [], []
    for im, (m, n) in enumerate(lists):
        obj = _boxes(rs, n, extent)
        cls = rs.randint(0, n_cls, n)
        cls[0] = 0
        if quantum:
            obj = np.round(obj / quantum) * quantum
        gt += [(im, int(c), o) for c, o in zip(cls, obj)]
        for c in range(n_cls):
            near = obj[rs.randint(0, n, m)] + rs.normal(0., extent / 40., (m, 4))
            cand = np.where((rs.rand(m) < 0.5)[:, None], near, _boxes(rs, m, extent))
            cand[:, 2:] = np.maximum(cand[:, 2:], cand[:, :2] + 1.)
            if quantum:
                cand = np.round(cand / quantum) * quantum
            boxes.append(cand[rs.permutation(m)])
            problems.append((im, c, m))
    case = _case(np.concatenate(boxes, 0) if boxes else [], problems, gt, n_cls, **kw)
    if with_area:
        a = case["args"]["gt_box"].astype(np.float64)
        case["args"]["gt_area"] = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) * rs.uniform(0.5, 1.1, a.shape[0])
    return case


GEOMETRY_LISTS = [(0, 1), (1, 2), (63, 3), (64, 64), (65, 65), (255, 130), (256, 1), (257, 2), (300, 3), (1, 3), (63, 130),
                  (300, 130), (64, 1), (65, 64), (40, 300)]
# every list length and object count the launch geometry turns on: the 64 lanes of a candidate scan, the 4 wavefronts that
# share the objects, the 256 threads of the reduction over the objects (300: a second trip), lists shorter than the objects


def geometry_case(**kw):
    return seeded_case(11, GEOMETRY_LISTS, n_cls=1, **kw)


def full_parameter_case():
    """T = 16, L = 8, A = 8: lists of 64 and 65 rows under limits below, on and above both lengths, and 0"""
    return seeded_case(12, [(64, 9), (65, 12), (64, 3)], n_cls=2, extent=700., with_area=True, others=True,
                       iou_thrs=tuple(np.linspace(0.05, 0.95, 16)), limits=(0, 1, 63, 64, 65, 66, 300, 1000), area_rng=None)


CONTESTED_SEED = 3


def contested_case(seed=CONTESTED_SEED):
    """a few centres; the objects are near-duplicates of the centres, the candidates jittered copies: many objects share a
    first choice. Asserted here, on the host: at least a quarter of the objects end with another match than their column
    argmax (the candidate that covers them best), so the matching had to look again for them."""
    from dana_amd import evaluate as E
    rs = np.random.RandomState(seed)
    centres = _boxes(rs, 6, 300., lo=40., hi=0.4)
    obj = centres[np.arange(30) % 6] + rs.normal(0., 1.0, (30, 4))
    cand = centres[rs.randint(0, 6, 48)] + rs.normal(0., 4.0, (48, 4))
    case = _case(cand, [(0, 0, 48)], [(0, 0, o) for o in obj], 1, iou_thrs=(0.5, 0.7, 0.9))
    a = case["args"]
    ref = E.proposal_recall_numpy(**a)
    first = E._iou_matrix(a["boxes"].astype(np.float64), a["gt_box"].astype(np.float64)).argmax(0)
    moved = ref["match"][0, 0] != first[ref["pair_gt"]]
    assert moved.mean() >= 0.25, "seed %d: only %.0f%% of the objects lost their first choice" % (seed, 100 * moved.mean())
    return case


def rpn_sized_case():
    """cfg.TRAIN.RPN_POST_NMS_TOP_N = 2000 rows in one list, five objects"""
    return seeded_case(13, [(2000, 5)], n_cls=1, extent=600., limits=(0, 300))


def three_class_case():
    """others=True with three classes; the objects of image 1 are all of class 0 (its other units are empty, its target
    unit covers everything), image 2 has one object"""
    case = seeded_case(14, [(40, 7), (30, 5), (20, 1)], n_cls=3, others=True, iou_thrs=(0.3, 0.5, 0.7), limits=(0, 10))
    a = case["args"]
    a["gt_cls"] = np.where(a["gt_img"] == 1, 0, a["gt_cls"])
    return case
