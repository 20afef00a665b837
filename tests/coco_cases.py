"""Inputs shared by tests/test_coco_eval_host.py and tests/test_gpu_coco_eval.py: the hand-worked COCO cases (their
expected values are spelled out in the host test) and the seeded generators. Not a test module."""
import numpy as np

HAND_THRS = (0.5, 0.75)

# name -> (detections (x1,y1,x2,y2,score), objects (x,y,w,h), iscrowd, ignore); one image, one class
HAND = {
    "crowd": ([(110, 110, 129, 129, .95), (150, 150, 169, 169, .92), (0, 0, 9, 9, .9), (300, 300, 319, 319, .6)],
              [(0, 0, 10, 10), (100, 100, 100, 100)], [0, 1], [0, 0]),
    "crowd flag off": ([(110, 110, 129, 129, .95), (150, 150, 169, 169, .92), (0, 0, 9, 9, .9), (300, 300, 319, 319, .6)],
                       [(0, 0, 10, 10), (100, 100, 100, 100)], [0, 0], [0, 0]),
    "maxDets": ([(300, 300, 319, 319, .9), (0, 0, 9, 9, .8), (50, 50, 59, 59, .7)], [(0, 0, 10, 10), (50, 50, 10, 10)],
                [0, 0], [0, 0]),
    "area": ([(400, 400, 449, 449, .95), (0, 0, 19, 19, .9), (100, 100, 299, 299, .8)],
             [(0, 0, 20, 20), (100, 100, 200, 200)], [0, 0], [0, 0]),
    "duplicates": ([(0, 0, 9, 9, .9), (0, 0, 9, 9, .8)], [(0, 0, 10, 10), (0, 0, 10, 10)], [0, 0], [0, 0]),
    "ignore preference": ([(0, 0, 9, 9, .9)], [(0, 0, 10, 16), (0, 0, 10, 11)], [0, 0], [0, 1]),
    "ignored only": ([(0, 0, 9, 9, .9), (40, 40, 49, 49, .8)], [(0, 0, 10, 11), (40, 40, 10, 10)], [0, 0], [1, 0]),
}


def hand_case(name):
    """-> dict of coco_numpy's array arguments for one hand case"""
    dets, objs, crowd, ignore = HAND[name]
    nd, ng = len(dets), len(objs)
    return dict(det=np.asarray(dets, np.float32), det_img=np.zeros(nd, np.int32), det_cls=np.zeros(nd, np.int32),
                gt_bbox=np.asarray(objs, np.float32), gt_img=np.zeros(ng, np.int32), gt_cls=np.zeros(ng, np.int32),
                gt_iscrowd=np.asarray(crowd, np.uint8), gt_area=None, gt_ignore=np.asarray(ignore, np.uint8))


def mean_valid(x):
    x = np.asarray(x)
    x = x[x > -1]
    return float(x.mean()) if x.size else -1.0


def disjoint_case(seed, n_img=5, n_cls=3, cells=4, dets_per_seg=8):
    """Ground truth of each (class, image): at most one box per cell of a cells x cells grid of 100-pixel cells, so
    pairwise disjoint. Detections: jittered copies of their segment's boxes, or boxes anywhere. Scores are pairwise
    distinct. -> (dict with xyxy ground truth `gt_box` and its COCO form `gt_bbox`, n_img, n_cls)"""
    rng = np.random.RandomState(seed)
    gb, gi, gc = [], [], []
    for c in range(n_cls):
        for i in range(n_img):
            for cell in rng.permutation(cells * cells)[:rng.randint(1, 7)]:
                x0, y0 = 100 * (cell % cells), 100 * (cell // cells)
                x, y = x0 + rng.randint(2, 30), y0 + rng.randint(2, 30)
                gb.append([x, y, x + rng.randint(25, 65), y + rng.randint(25, 65)])  # stays inside its cell
                gi.append(i)
                gc.append(c)
    gb = np.asarray(gb, np.float32)
    gi, gc = np.asarray(gi, np.int32), np.asarray(gc, np.int32)
    db, di, dc = [], [], []
    for c in range(n_cls):
        for i in range(n_img):
            mine = np.nonzero((gi == i) & (gc == c))[0]
            for _ in range(dets_per_seg):
                if rng.rand() < 0.6:
                    b = gb[mine[rng.randint(mine.size)]] + rng.uniform(-7, 7, 4)
                else:
                    x, y = rng.uniform(0, 330, 2)
                    b = np.asarray([x, y, x + rng.uniform(20, 70), y + rng.uniform(20, 70)])
                db.append(b)
                di.append(i)
                dc.append(c)
    n = len(db)
    score = ((rng.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)
    assert np.unique(score).size == n
    perm = rng.permutation(n)
    det = np.concatenate((np.asarray(db, np.float32), score[:, None]), 1).astype(np.float32)[perm]
    bbox = np.stack((gb[:, 0], gb[:, 1], gb[:, 2] - gb[:, 0] + 1, gb[:, 3] - gb[:, 1] + 1), 1).astype(np.float32)
    return dict(det=det, det_img=np.asarray(di, np.int32)[perm], det_cls=np.asarray(dc, np.int32)[perm], gt_box=gb,
                gt_bbox=bbox, gt_img=gi, gt_cls=gc), n_img, n_cls


def mixed_case(seed, n_img, n_cls, dets_per_seg, gts_per_seg, crowd=0.15, ignore=0.1, tie_scores=False, seg_area=True):
    """Random objects of sizes from small to large (overlapping freely), some crowd, some ignore; annotation areas are a
    share of w*h when seg_area. Detections: jittered copies of their segment's objects 60 % of the time, boxes inside a
    crowd region sometimes, else anywhere. dets_per_seg / gts_per_seg are functions of (class, image)."""
    rng = np.random.RandomState(seed)
    sizes = (8, 20, 50, 80, 120, 220)
    gb, gi, gc = [], [], []
    for c in range(n_cls):
        for i in range(n_img):
            for _ in range(gts_per_seg(c, i)):
                x, y = rng.randint(0, 300, 2)
                gb.append([x, y, sizes[rng.randint(len(sizes))] + rng.randint(0, 9), sizes[rng.randint(len(sizes))] + rng.randint(0, 9)])
                gi.append(i)
                gc.append(c)
    gb = np.asarray(gb, np.float32).reshape(-1, 4)
    gi, gc = np.asarray(gi, np.int32), np.asarray(gc, np.int32)
    g = gb.shape[0]
    iscrowd = (rng.rand(g) < crowd).astype(np.uint8)
    ign = (rng.rand(g) < ignore).astype(np.uint8)
    area = gb[:, 2].astype(np.float64) * gb[:, 3] * (rng.uniform(0.4, 1.0, g) if seg_area else 1.0)
    db, di, dc = [], [], []
    for c in range(n_cls):
        for i in range(n_img):
            mine = np.nonzero((gi == i) & (gc == c))[0]
            for _ in range(dets_per_seg(c, i)):
                u = rng.rand()
                if mine.size and u < 0.6:
                    x, y, w, h = gb[mine[rng.randint(mine.size)]]
                    b = np.asarray([x, y, x + w - 1, y + h - 1]) + rng.uniform(-0.12, 0.12, 4) * min(w, h)
                elif mine.size and u < 0.75 and iscrowd[mine].any():
                    x, y, w, h = gb[mine[iscrowd[mine] == 1][0]]
                    fx, fy = rng.uniform(0, 0.5, 2)
                    b = np.asarray([x + fx * w, y + fy * h, x + (fx + 0.45) * w, y + (fy + 0.45) * h])
                else:
                    x, y = rng.uniform(0, 300, 2)
                    b = np.asarray([x, y, x + rng.uniform(6, 200), y + rng.uniform(6, 200)])
                db.append(b)
                di.append(i)
                dc.append(c)
    n = len(db)
    score = ((rng.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)
    if tie_scores:
        score = (np.floor(score * 4) / 4).astype(np.float32)  # four distinct values: image index and arrival decide
    perm = rng.permutation(n)
    det = np.concatenate((np.asarray(db, np.float32).reshape(-1, 4), score[:, None]), 1).astype(np.float32)[perm]
    return dict(det=det, det_img=np.asarray(di, np.int32)[perm], det_cls=np.asarray(dc, np.int32)[perm], gt_bbox=gb,
                gt_img=gi, gt_cls=gc, gt_iscrowd=iscrowd, gt_area=area, gt_ignore=ign)
