"""Composed queries in the episode assembler (csrc/episode.hip's *_composed launches through pipeline.plan_episode /
EpisodeAssembler) on the small pool of test_gpu_episode_assembler.py. Everything is compared bit for bit with code the
feature does not touch:

  * pixels   a part's rectangle of im_data == the same rectangle cut by slicing from a plain (or, with a colour map,
             augmented) one-query `crop` plan assembled on its own; painted over each other in order on the host (`_paint`)
  * boxes    == pipeline.composed_boxes_numpy; where nothing overlaps also == the per-part plain outputs moved by a float32
             add; one part at (0, 0) == the plain launches outright
  * a visibility threshold is only ever tested where every box keeps |(seen - hidden) - f * full| >= VIS_GAP * full
    (the argument of test_gpu_episode_augment.py: closer than that a case tests roundings, not the rule); `_keeps_the_gap`
    checks it on the host in float64 before anything runs on the device

One case needs a pool row with more than 64 boxes, which the four rows do not have: it appends a fifth row to the same
four (`MANY`)."""
import re

import numpy as np
import pytest
import torch

from test_gpu_episode_assembler import MEANS, QUERY_CASES, SMALL, SUPPORTS, make_pool, same
from test_gpu_episode_augment import VIS_GAP, _distorted_pool

pytestmark = pytest.mark.gpu

HW = (48, 64)


def _assemble(dev, pool, plan, ws=0, nb=8, support_size=32):
    """-> im_data, im_info, gt_boxes, num_boxes, support_ims, all_cls_gt_boxes, all_cls_num_boxes from holders full of 7"""
    from dana_amd import pipeline as PL
    H, W = plan.holder_hw
    hold = PL.EpisodeHolders(plan.batch, 1, ws, H, W, dev, support_size=support_size, max_num_box=nb)
    for t in hold.tensors():
        t.fill_(7)
    asm = PL.EpisodeAssembler(pool, hold, pixel_means=MEANS)
    asm.all_cls_gt_boxes.fill_(7)
    asm.all_cls_num_boxes.fill_(7)
    out = asm.assemble(plan)
    torch.cuda.synchronize()
    return list(out) + [asm.all_cls_num_boxes]


def _paint(dev, pool, parts, hw, target, pools=None):
    """im_data [3][H][W] of one composed query from one-query plans of code that knows no parts, painted in order by slicing.
    pools[k]: another pool to take part k from, through the plain launches (its colour map is then left out)"""
    from dana_amd import pipeline as PL
    want = torch.zeros((3,) + tuple(hw), device=dev)
    for k, part in enumerate(parts):
        if part.get("erase") is not None:
            dy, dx, h, w = part["erase"]
            want[:, dy:dy + h, dx:dx + w] = 0
            continue
        src, color = (pool, part.get("color")) if pools is None or pools[k] is None else (pools[k], None)
        (_, _, h, w), (dy, dx) = part["crop"], part["at"]
        q = dict(row=part["row"], pos_cls=1, crop=part["crop"], target_size=part.get("target_size", target))
        if color is not None:
            q["color"] = color
        plan = PL.plan_episode(src, [q], holder_hw=hw, target_size=target)
        assert not plan.composed and plan.augmented == (color is not None)
        want[:, dy:dy + h, dx:dx + w] = _assemble(dev, src, plan, nb=1)[0][0, :, :h, :w]
    return want


def _keeps_the_gap(plan, pool):
    """every box of every composed query with a threshold, in float64: far enough from it (see the head of the file)"""
    for q in plan.queries:
        f = q.get("min_visible") or 0.0
        if "parts" not in q or f <= 0:
            continue
        rects = [(p["dx"], p["dy"], p["dx"] + p["w"] - 1, p["dy"] + p["h"] - 1) for p in q["parts"]]
        for k, p in enumerate(q["parts"]):
            if p["row"] < 0:
                continue
            for box in np.asarray(pool.row_boxes(p["row"]), dtype=np.float64)[np.asarray(p["order"], dtype=np.int64)]:
                u = box[:4] * p["im_scale"] - np.array([p["x_s"], p["y_s"], p["x_s"], p["y_s"]], dtype=np.float64)
                v = np.clip(u, 0, [p["w"] - 1, p["h"] - 1, p["w"] - 1, p["h"] - 1])
                if v[0] == v[2] or v[1] == v[3]:
                    continue
                t = v + [p["dx"], p["dy"], p["dx"], p["dy"]]
                hidden = sum(max(min(t[2], r[2]) - max(t[0], r[0]), 0) * max(min(t[3], r[3]) - max(t[1], r[1]), 0)
                             for r in rects[k + 1:])
                full, seen = (u[2] - u[0]) * (u[3] - u[1]), (v[2] - v[0]) * (v[3] - v[1])
                if abs((seen - hidden) - f * full) < VIS_GAP * full:
                    return False
    return True


def _check(dev, pool, queries, hw=HW, target=48, nb=8, pools=None):
    """plan, assemble, compare: the composed queries' pixels with `_paint`, all boxes with the numpy restatement, im_info.
    pools: {b: per-part pools} for `_paint` -> (plan, outputs)"""
    from dana_amd import pipeline as PL
    plan = PL.plan_episode(pool, queries, holder_hw=hw, target_size=target)
    assert plan.composed and _keeps_the_gap(plan, pool)
    got = _assemble(dev, pool, plan, nb=nb)
    fs, n_fs, al, n_al = plan.boxes_numpy(pool, nb)
    print("num_boxes", got[3].tolist(), got[6].tolist(), "expected", n_fs.tolist(), n_al.tolist())
    assert got[3].tolist() == n_fs.tolist() and got[6].tolist() == n_al.tolist()
    assert got[2].cpu().numpy().tobytes() == fs.tobytes() and got[5].cpu().numpy().tobytes() == al.tobytes()
    for b, q in enumerate(queries):
        if q.get("parts") is None:
            continue
        want = _paint(dev, pool, q["parts"], hw, target, None if pools is None else pools.get(b))
        assert torch.equal(got[0][b], want), "query %d: %d pixels differ" % (b, int((got[0][b] != want).sum()))
        assert got[1][b].tolist() == [hw[0], hw[1], np.float32(plan.queries[b]["im_scale"])]
    return plan, got


# ---- 1. one part at (0, 0) is the plain crop -------------------------------------------------------------------------------
def _neg():
    m = -np.eye(3, 4, dtype=np.float32)
    m[:, 3] = 255
    return m


CROPS = [dict(row=1, pos_cls=1, crop=(5, 30, 40, 30), min_visible=0.3),   # 48 x 69 prepared: an inner window
         dict(row=3, pos_cls=1, crop=(8, 9, 40, 60)),                     # the flipped twin, to its last row and column
         dict(row=2, pos_cls=1, crop=(30, 10, 30, 38), min_visible=0.5, color=_neg(), order=[1, 2, 0]),
         dict(row=0, pos_cls=2, crop=(0, 3, 48, 64), order=[1, 0])]       # upscaled 9.6 x: a window that IS the holder


@pytest.mark.parametrize("which", ["augmented", "plain"])
def test_one_part_at_the_origin_equals_the_plain_crop(dev, which):
    """all seven outputs, against the augmented launches (two thresholds and a colour map) and against the plain ones"""
    from dana_amd import pipeline as PL
    pool, _ = make_pool(dev, SMALL)
    crops = CROPS if which == "augmented" else [{k: v for k, v in q.items() if k not in ("min_visible", "color")} for q in CROPS]
    sups = SUPPORTS + SUPPORTS[:2]
    plain = PL.plan_episode(pool, crops, sups, holder_hw=HW, target_size=48, support_size=32)
    comp = PL.plan_episode(pool, [dict(q, at=(0, 0)) for q in crops], sups, holder_hw=HW, target_size=48, support_size=32)
    assert comp.composed and not comp.augmented and not plain.composed and plain.augmented == (which == "augmented")
    assert comp.max_parts == 1 and _keeps_the_gap(comp, pool)
    got, want = _assemble(dev, pool, comp, ws=2, nb=4), _assemble(dev, pool, plain, ws=2, nb=4)
    same(got, want)
    assert float(got[0].abs().max()) > 1 and int(got[3].sum()) > 0 and int(got[6].sum()) > 0 and not (got[4] == 7).any()
    if which == "augmented":  # the thresholds did drop something
        assert got[6].tolist() != _assemble(dev, pool, PL.plan_episode(pool, [dict(q, at=(0, 0), min_visible=None) for q in crops],
                                                                       holder_hw=HW, target_size=48), nb=4)[6].tolist()


# ---- 2. queries that are not composed, inside a composed batch ---------------------------------------------------------------
MOSAIC_SIZES = [48, 32, 48, 48]  # row 0 upscaled 9.6 x, row 1 downscaled to 32 x 46, row 2 at scale 1, row 3 a flipped twin


def _mosaic(**kw):
    from dana_amd import pipeline as PL
    pool = PL.ImagePool()
    for spec in SMALL:  # a host twin of the pool's tables: the helpers read sizes and boxes only
        pool.add_flipped(spec[1], spec[2]) if spec[0] == "flip" else pool.add(np.zeros((spec[0], spec[1], 3), np.uint8), spec[2])
    return PL.mosaic_query(pool.freeze(), [0, 1, 2, 3], (19, 29), HW, target_size=MOSAIC_SIZES, **kw)


@pytest.mark.parametrize("case", ["up_crop_flip", "down_pad_both"])
@pytest.mark.parametrize("augment", [False, True])
def test_plain_queries_in_a_composed_batch_keep_their_bits(dev, case, augment):
    from dana_amd import pipeline as PL
    target, hw, queries = QUERY_CASES[case]
    if augment:
        queries = [dict(q, min_visible=0.3, color=_neg() if b != 1 else None) for b, q in enumerate(queries)]
    pool, _ = make_pool(dev, SMALL)
    plain = PL.plan_episode(pool, queries, holder_hw=hw, target_size=target)
    mixed_q = [queries[0], _mosaic(min_visible=0.3), queries[1], queries[2]]
    mixed = PL.plan_episode(pool, mixed_q, holder_hw=hw, target_size=target)
    assert mixed.composed and not plain.composed and plain.augmented == augment and mixed.max_parts == 4
    _, got = _check(dev, pool, mixed_q, hw=hw, target=target, nb=4)
    want = _assemble(dev, pool, plain, nb=4)
    keep = torch.tensor([0, 2, 3], device=dev)
    same([t[keep] for t in got[:4] + got[5:]], want[:4] + want[5:])
    assert int(want[6].sum()) > 0 and float(want[0].abs().max()) > 1


# ---- 3. mosaic ---------------------------------------------------------------------------------------------------------------
def test_mosaic_quadrants_and_boxes(dev):
    """four parts meeting at (19, 29): each quadrant is the one-query crop plan's window, and since nothing overlaps the
    boxes are the one-query plans' boxes moved to the quadrant by a float32 add, in part order"""
    from dana_amd import pipeline as PL
    pool, _ = make_pool(dev, SMALL)
    q = _mosaic(min_visible=0.3, pos_cls=1)
    assert [p["at"] for p in q["parts"]] == [(0, 0), (0, 29), (19, 0), (19, 29)]
    assert [p["crop"][2:] for p in q["parts"]] == [(19, 29), (19, 35), (29, 29), (29, 35)]
    plan, got = _check(dev, pool, [q], nb=8)
    assert [round(p["im_scale"], 3) for p in plan.queries[0]["parts"]] == [9.6, 0.865, 1.0, 1.297]
    assert not (got[0] == 7).any() and float(got[0].abs().max()) > 1
    rows_all, rows_fs = [], []
    for part in q["parts"]:
        one = PL.plan_episode(pool, [dict(row=part["row"], crop=part["crop"], target_size=part["target_size"], pos_cls=1,
                                          min_visible=0.3)], holder_hw=HW, target_size=48)
        out = _assemble(dev, pool, one, nb=8)
        shift = torch.tensor([part["at"][1], part["at"][0], part["at"][1], part["at"][0], 0], dtype=torch.float32, device=dev)
        rows_all.append(out[5][0, :int(out[6][0])] + shift)
        rows_fs.append(out[2][0, :int(out[3][0])] + shift)
    for rows, boxes, count in ((rows_all, got[5], got[6]), (rows_fs, got[2], got[3])):
        rows = torch.cat(rows)[:8]
        assert int(count[0]) == rows.size(0) >= 2 and torch.equal(boxes[0, :rows.size(0)], rows) and not boxes[0, rows.size(0):].any()


# ---- 4. painting order -------------------------------------------------------------------------------------------------------
def test_later_parts_paint_over_earlier_ones(dev):
    pool, _ = make_pool(dev, SMALL)
    a = dict(row=1, crop=(0, 0, 30, 40), at=(2, 3))
    b = dict(row=2, crop=(5, 5, 25, 30), at=(20, 30))  # overlap: rows 20..31, columns 30..42
    _, ab = _check(dev, pool, [dict(parts=[a, b], pos_cls=1)])
    _, ba = _check(dev, pool, [dict(parts=[b, a], pos_cls=1)])
    only_a = _paint(dev, pool, [a], HW, 48)
    only_b = _paint(dev, pool, [b], HW, 48)
    lap = (slice(None), slice(20, 32), slice(30, 43))
    assert torch.equal(ab[0][0][lap], only_b[lap]) and torch.equal(ba[0][0][lap], only_a[lap])
    assert not torch.equal(only_a[lap], only_b[lap]) and (only_a[lap] != 0).all() and (only_b[lap] != 0).all()
    outside = torch.ones(HW, dtype=torch.bool, device=dev)
    outside[2:32, 3:43] = False
    outside[20:45, 30:60] = False
    assert int(outside.sum()) > 0 and not ab[0][0][:, outside].any() and not ba[0][0][:, outside].any()  # the 7s are gone


# ---- 5. erase ------------------------------------------------------------------------------------------------------------------
def test_erase_part(dev):
    """row 1's window (5, 9, 40, 60) under an erased [0, 24) x [0, 32): box 0 lies under it entirely, box 1 keeps 0.65 of its
    area and box 2 (the whole frame, cut by the window) 0.46"""
    from dana_amd import pipeline as PL
    pool, _ = make_pool(dev, SMALL)
    base = dict(row=1, crop=(5, 9, 40, 60), at=(0, 0))
    plain = _assemble(dev, pool, PL.plan_episode(pool, [dict(row=1, pos_cls=1, crop=(5, 9, 40, 60))], holder_hw=HW, target_size=48))
    for f, count in ((0.5, 1), (0.0, 3)):
        _, got = _check(dev, pool, [dict(parts=[base, dict(erase=(0, 0, 24, 32))], pos_cls=1, min_visible=f)])
        assert got[6].tolist() == [count]
        assert not got[0][0, :, :24, :32].any()
        keep = torch.ones(HW, dtype=torch.bool, device=dev)
        keep[:24, :32] = False
        assert torch.equal(got[0][0][:, keep], plain[0][0][:, keep]) and plain[0][0, :, :24, :32].abs().min() > 0
        if f == 0.0:  # no rule: the boxes of the plain crop, covered or not
            same(got[1:4] + got[5:], plain[1:4] + plain[5:])


# ---- 6. the occlusion rule -----------------------------------------------------------------------------------------------------
# row 1 at target 37 is at scale 1 exactly (37 x 53 prepared); its whole frame at (2, 5) puts box 0 (3, 4, 30, 20) at
# t = (8, 6, 35, 22), area 432; boxes 1 and 2 ride along and are checked against the restatement like box 0
BASE = dict(row=1, crop=(0, 0, 37, 53), at=(2, 5), target_size=37)
OCCLUSION = {
    "no cover": ([BASE], 0.5, 3),
    "left": ([BASE, dict(erase=(0, 0, 30, 21))], 0.5, None),                          # x [0, 20]: 12 * 16 of 432 hidden
    "right, by a source part": ([BASE, dict(row=0, crop=(0, 0, 30, 30), at=(0, 25))], 0.5, None),  # x [25, 54]: 10 * 16 hidden
    "top": ([BASE, dict(erase=(0, 0, 14, 64))], 0.5, None),                           # y [0, 13]: 27 * 7 hidden
    "bottom": ([BASE, dict(erase=(13, 0, 30, 64))], 0.5, None),                       # y [13, 42]: 27 * 9 hidden: 0.4375 left
    "full": ([BASE, dict(erase=(0, 0, 48, 64))], 0.01, 0),
    # two covers that overlap each other: the union hides 13 * 16 = 208 (0.52 left: kept at 0.5), the sum hides
    # 208 + 11 * 16 = 384 (0.11 left: dropped). The rule is the sum.
    "two covers, summed": ([dict(BASE, order=[0]), dict(erase=(0, 0, 30, 22)), dict(erase=(0, 0, 30, 20))], 0.5, 0),
    "two covers, f below the sum": ([dict(BASE, order=[0]), dict(erase=(0, 0, 30, 22)), dict(erase=(0, 0, 30, 20))], 0.1, 1),
    # clamped by its own window (x [10, 39]: u = (-7, 4, 20, 20), v = (0, 4, 20, 20), 320 of 432) and covered (5 * 16 = 80)
    "clamped and covered, kept": ([dict(BASE, crop=(0, 10, 37, 30), order=[0]), dict(erase=(0, 0, 30, 11))], 0.5, 1),
    "clamped and covered, dropped": ([dict(BASE, crop=(0, 10, 37, 30), order=[0]), dict(erase=(0, 0, 30, 11))], 0.6, 0),
    "clamped, not covered": ([dict(BASE, crop=(0, 10, 37, 30), order=[0])], 0.7, 1),  # 320 / 432 = 0.74
}


def test_occlusion_cases_keep_the_gap():
    """the condition of the cases below, asserted before anything runs on the device (host tables only)"""
    from dana_amd import pipeline as PL
    pool = PL.ImagePool()
    for spec in SMALL:
        pool.add_flipped(spec[1], spec[2]) if spec[0] == "flip" else pool.add(np.zeros((spec[0], spec[1], 3), np.uint8), spec[2])
    pool.freeze()
    for name, (parts, f, _) in OCCLUSION.items():
        plan = PL.plan_episode(pool, [dict(parts=parts, pos_cls=1, min_visible=f)], holder_hw=HW, target_size=48)
        assert _keeps_the_gap(plan, pool), name
    # and the check does refuse a case on the threshold: "top" with one more row hides 27 * 8 = 216 = half of box 0
    on_it = PL.plan_episode(pool, [dict(parts=[BASE, dict(erase=(0, 0, 15, 64))], pos_cls=1, min_visible=0.5)], holder_hw=HW)
    assert not _keeps_the_gap(on_it, pool)


@pytest.mark.parametrize("name", sorted(OCCLUSION))
def test_occlusion_rule_equals_the_numpy_restatement(dev, name):
    from dana_amd import pipeline as PL
    parts, f, count = OCCLUSION[name]
    pool, _ = make_pool(dev, SMALL)
    plan, got = _check(dev, pool, [dict(parts=parts, pos_cls=1, min_visible=f)])
    ruleless = PL.plan_episode(pool, [dict(parts=parts, pos_cls=1)], holder_hw=HW, target_size=48).boxes_numpy(pool, 8)
    print(name, "kept", got[6].tolist(), "without the rule", ruleless[3].tolist())
    if count is not None:
        assert got[6].tolist() == [count]
    if name == "no cover":
        assert got[5][0, 0].tolist() == [8, 6, 35, 22, 1]
    if name in ("left", "right, by a source part", "top"):  # box 0 stays, in front
        assert got[5][0, 0].tolist() == [8, 6, 35, 22, 1]
    if name == "bottom":
        assert int(got[6][0]) < int(ruleless[3][0]) and got[5][0, 0].tolist() != [8, 6, 35, 22, 1]
    if name == "two covers, summed":
        one_cover = PL.plan_episode(pool, [dict(parts=parts[:2], pos_cls=1, min_visible=f)], holder_hw=HW, target_size=48)
        assert one_cover.boxes_numpy(pool, 8)[3].tolist() == [1]  # the union of the two covers IS the first: it alone keeps the box


# ---- 7. colour per part ----------------------------------------------------------------------------------------------------------
def test_a_parts_colour_map_stays_in_its_part(dev):
    pool, src = make_pool(dev, SMALL)
    pool2 = _distorted_pool(dev, src, lambda im: 255 - im)
    for k in (1, 3):  # the downscaled part; the flipped twin
        q = _mosaic(colors=[_neg() if j == k else None for j in range(4)], min_visible=0.3)
        _, got = _check(dev, pool, [q], pools={0: [pool2 if j == k else None for j in range(4)]})
        _, bare = _check(dev, pool, [_mosaic(min_visible=0.3)])
        (dy, dx), (_, _, h, w) = q["parts"][k]["at"], q["parts"][k]["crop"]
        inside = torch.zeros(HW, dtype=torch.bool, device=dev)
        inside[dy:dy + h, dx:dx + w] = True
        assert torch.equal(got[0][0][:, ~inside], bare[0][0][:, ~inside]) and (got[0][0][:, inside] != bare[0][0][:, inside]).any()
        same(got[1:4] + got[5:], bare[1:4] + bare[5:])  # colour leaves the boxes alone


# ---- 8. the edges of the launch geometry -------------------------------------------------------------------------------------------
def _many():
    """the fifth row: 40 x 50 (scale 1 at target 40) with 100 boxes of which every 16th is not degenerate, of class 2 and 1
    in turn. Kept boxes fall in both 64-lane passes of a part that walks all of them."""
    b = np.zeros((100, 5), dtype=np.float32)
    b[:, 0] = b[:, 2] = np.arange(100) % 40
    b[:, 1], b[:, 3] = 1, 9
    for n, k in enumerate(range(5, 100, 16)):  # 5, 21, 37, 53, 69, 85
        b[k, :4] = (2 + 3 * n, 4 + n, 14 + 3 * n, 20 + n)
    b[:, 4] = np.where((np.arange(100) // 16) % 2 == 0, 2, 1)
    return (40, 50, b.tolist())


MANY = SMALL + [_many()]


def _sixteen():
    """sixteen parts on a 4 x 4 grid of 11 x 15 cells, sizes up to 9 x 13 so that neighbours in a row overlap by a column or
    two now and then; part 7 is an erase, part 15 ends on the holder's last row and column"""
    parts = []
    for k in range(16):
        dy, dx = (k // 4) * 11 + k % 3, (k % 4) * 15 + (k * 5) % 4
        h, w = 5 + k % 5, 9 + (k * 3) % 5
        if k == 15:
            dy, dx = 48 - h, 64 - w
        if k == 7:
            parts.append(dict(erase=(dy, dx, h, w)))
        else:
            parts.append(dict(row=k % 4, crop=(2 * k, (7 * k) % 30, h, w), at=(dy, dx), target_size=[48, 40, 48, 36][k % 4]))
    return parts


EDGES = {
    # a column 1 pixel wide on the last column, a row 1 pixel high on the last row, a part into the bottom-right corner
    "thin parts and the last row and column": (HW, 8, [dict(parts=[
        dict(row=1, crop=(5, 9, 40, 60), at=(0, 0)), dict(row=2, crop=(3, 7, 20, 1), at=(10, 63)),
        dict(row=0, crop=(4, 4, 1, 30), at=(47, 0)), dict(row=3, crop=(8, 9, 10, 12), at=(38, 52))], pos_cls=1, min_visible=0.3)]),
    # 37 * 53 = 1961 pixels: seven full workgroups and 169 threads of an eighth; B = 1
    "a holder that is no multiple of 256": ((37, 53), 8, [dict(parts=[
        dict(row=1, crop=(0, 0, 37, 53), at=(0, 0), target_size=37), dict(row=2, crop=(9, 9, 12, 31), at=(25, 22))],
        pos_cls=1, min_visible=0.2)]),
    # B = 3 with tables of 16, 1 and 2 parts at a stride of 16 records
    "sixteen parts": (HW, 8, [dict(parts=_sixteen(), pos_cls=1, min_visible=0.05), dict(row=2, ratio=1.0, pos_cls=1, order=[2, 0, 1]),
                              dict(parts=[dict(row=3, crop=(0, 0, 48, 64), at=(0, 0)), dict(erase=(40, 0, 8, 64))], pos_cls=2)]),
    # 100 + 70 + 3 boxes in order: part 0's kept boxes sit at 5, 21, 37, 53 (first pass) and 69, 85 (second); part 1 walks
    # the same row backwards from 69 and brings the all-class list past max_num_box = 8 in its middle, the class-1 list not
    "two passes in a part, the cut in the middle of the next": (HW, 8, [dict(parts=[
        dict(row=4, crop=(0, 0, 40, 50), at=(0, 0), target_size=40),
        dict(row=4, crop=(0, 0, 40, 50), at=(8, 14), target_size=40, order=list(range(69, -1, -1))),
        dict(row=2, crop=(0, 0, 6, 6), at=(42, 58))], pos_cls=2)]),
    # part 0 lies under part 1 entirely: all its boxes go, part 1's stay and are the first rows
    "a part whose boxes all go, then one whose boxes stay": (HW, 8, [dict(parts=[
        dict(row=1, crop=(0, 0, 37, 53), at=(2, 5), target_size=37), dict(row=3, crop=(0, 0, 37, 53), at=(2, 5), target_size=37)],
        pos_cls=1, min_visible=0.05)]),
}


def test_edge_cases_keep_the_gap():
    from dana_amd import pipeline as PL
    pool = PL.ImagePool()
    for spec in MANY:
        pool.add_flipped(spec[1], spec[2]) if spec[0] == "flip" else pool.add(np.zeros((spec[0], spec[1], 3), np.uint8), spec[2])
    pool.freeze()
    for name, (hw, _, queries) in EDGES.items():
        assert _keeps_the_gap(PL.plan_episode(pool, queries, holder_hw=hw, target_size=48), pool), name


@pytest.mark.parametrize("name", sorted(EDGES))
def test_launch_geometry_edges(dev, name):
    hw, nb, queries = EDGES[name]
    pool, _ = make_pool(dev, MANY)
    assert np.array_equal(pool.meta[:4], make_pool(dev, SMALL)[0].meta)  # the four rows are the four rows
    plan, got = _check(dev, pool, queries, hw=hw, nb=nb)
    assert float(got[0].abs().max()) > 1
    if name == "sixteen parts":
        assert plan.max_parts == 16 and plan.batch == 3 and int(got[6][0]) >= 2 and not got[0][2, :, 40:].any()
    if name.startswith("two passes"):
        al = plan.boxes_numpy(pool, 200)
        assert al[3].tolist() == [6 + 5 + 1] and 0 < al[1][0] < 8 and got[6].tolist() == [8]  # cut inside part 1; class 2 not cut
        assert got[5][0, 5, 0] == 2 + 3 * 5 and got[5][0, 6, 0] == 2 + 3 * 4 + 14  # box 85 of part 0, then box 69 of part 1
    if name.startswith("a part whose boxes all go"):
        assert got[6].tolist() == [2] and got[5][0, 0].tolist() == [27, 6, 54, 22, 1]  # the twin's (22, 4, 49, 20) at (2, 5)


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
def _entry_args(dev, pool, plan, nb=4):
    B, (H, W) = plan.batch, plan.holder_hw
    out = dict(im=torch.full((B, 3, H, W), 7.0, device=dev), info=torch.full((B, 3), 7.0, device=dev),
               fs=torch.full((B, nb, 5), 7.0, device=dev), al=torch.full((B, nb, 5), 7.0, device=dev),
               n_fs=torch.full((B,), -1, dtype=torch.long, device=dev), n_al=torch.full((B,), -1, dtype=torch.long, device=dev))
    return out, torch.from_numpy(plan.words).to(dev)


def _call_composed(dev, pool, plan, out, d_plan, n_words, c_off, max_parts, nb=4):
    """both composed entry points with these numbers -> their return codes"""
    import ctypes
    from dana_amd._lib import lib
    means = (ctypes.c_float * 3)(*[float(m) for m in MEANS])
    stream = torch.cuda.current_stream().cuda_stream
    B, (H, W) = plan.batch, plan.holder_hw
    rc_q = lib().query("dana_episode_queries_composed", pool.data.data_ptr(), pool.data.numel(), pool.d_offsets.data_ptr(),
                       pool.d_meta.data_ptr(), len(pool), d_plan.data_ptr(), n_words, c_off, max_parts, B,
                       ctypes.cast(means, ctypes.c_void_p), out["im"].data_ptr(), H, W, out["info"].data_ptr(), stream)
    rc_b = lib().query("dana_episode_boxes_composed", pool.d_boxes.data_ptr(), len(pool.boxes), pool.d_meta.data_ptr(), len(pool),
                       d_plan.data_ptr(), n_words, c_off, max_parts, B, nb, out["fs"].data_ptr(), out["n_fs"].data_ptr(),
                       out["al"].data_ptr(), out["n_al"].data_ptr(), stream)
    torch.cuda.synchronize()
    return rc_q, rc_b


def test_entry_points_refuse_a_bad_section(dev):
    from dana_amd import pipeline as PL
    from dana_amd._lib import lib
    pool, _ = make_pool(dev, SMALL)
    plan = PL.plan_episode(pool, [_mosaic(min_visible=0.3), dict(row=2, ratio=1.0, pos_cls=1)], holder_hw=HW, target_size=48)
    n, c, m = int(plan.words.size), plan.c_off, plan.max_parts
    n_fit = c + 2 * PL.EP_CWORDS + 2 * m * PL.EP_PWORDS  # where the part records end; the parts' box orders follow
    assert m == 4 and n_fit < n
    out, d_plan = _entry_args(dev, pool, plan)
    bad = {"the parts section does not fit": (n_fit - 1, c, m, "does not fit the plan"),
           "the section does not fit at a larger stride": (n_fit, c, m + 1, "does not fit the plan"),
           "an odd offset": (n, c + 1, m, "odd word"),
           "a negative offset": (n, -2, m, "odd word|does not fit"),
           "a part count of 0": (n, c, 0, "part count outside 1..16"),
           "a part count of 17": (n + 100000, c, 17, "part count outside 1..16")}
    for name, (n_words, c_off, max_parts, message) in bad.items():
        rc = _call_composed(dev, pool, plan, out, d_plan, n_words, c_off, max_parts)
        assert rc[0] != 0 and rc[1] != 0, name
        assert re.search(message, lib().cdll.dana_last_error().decode()), (name, lib().cdll.dana_last_error().decode())
        assert all(bool((t == 7).all()) for t in (out["im"], out["info"], out["fs"], out["al"])), name
        assert bool((out["n_fs"] == -1).all()) and bool((out["n_al"] == -1).all()), name
    # the same buffers with the plan's own numbers
    assert _call_composed(dev, pool, plan, out, d_plan, n, c, m) == (0, 0)
    want = _assemble(dev, pool, plan, nb=4)
    same([out["im"], out["info"], out["fs"], out["n_fs"], out["al"], out["n_al"]], want[:4] + want[5:])


@pytest.mark.parametrize("row", [4, 99, -3])
def test_a_part_row_outside_the_pool_paints_zeros_and_has_no_boxes(dev, row):
    from dana_amd import pipeline as PL
    pool, _ = make_pool(dev, SMALL)
    q = _mosaic(min_visible=0.3)
    plan = PL.plan_episode(pool, [q], holder_hw=HW, target_size=48)
    bare = _assemble(dev, pool, plan)
    rec = plan.c_off + PL.EP_CWORDS + 1 * PL.EP_PWORDS  # part 1: the top-right quadrant, three of the four kept boxes
    assert plan.words[rec + PL.P_ROW] == 1
    plan.words[rec + PL.P_ROW] = row
    got = _assemble(dev, pool, plan)
    inside = torch.zeros(HW, dtype=torch.bool, device=dev)
    inside[:19, 29:] = True
    assert not got[0][0][:, inside].any() and torch.equal(got[0][0][:, ~inside], bare[0][0][:, ~inside]) and bare[0][0][:, inside].all()
    host = plan.queries[0]
    parts = [dict(p, boxes=None if k == 1 else pool.row_boxes(p["row"])) for k, p in enumerate(host["parts"])]
    fs, n_fs, al, n_al = PL.composed_boxes_numpy(parts, host["pos_cls"], 8, min_visible=0.3)
    assert got[6].tolist() == [n_al] and got[3].tolist() == [n_fs] and n_al < int(bare[6][0])
    assert got[5][0].cpu().numpy().tobytes() == al.tobytes() and got[2][0].cpu().numpy().tobytes() == fs.tobytes()
