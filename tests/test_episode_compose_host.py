"""Host side of composed queries in the episode assembler (dana_amd/pipeline.py): composed_boxes_numpy on answers worked by
hand, mosaic_query against a brute-force tiling of a small holder, paste_part, the draw helpers' draw counts, the words of
a composed plan, every refusal, and the words of plain and augmented plans, which must not have moved
(tests/golden/episode_plan_words.npy was written before either feature existed). No device."""
import os

import numpy as np
import pytest

from dana_amd import pipeline as PL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "episode_plan_words.npy")


def _im(h, w):
    return np.zeros((h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def pool():
    p = PL.ImagePool()  # the pool of test_episode_plan_host.py
    p.add(_im(5, 7), [[1, 1, 4, 3, 2]])
    p.add(_im(37, 53), [[3, 4, 30, 20, 1], [10, 5, 50, 36, 2]])
    p.add(_im(64, 48), [[2, 2, 40, 60, 1]])
    p.add_flipped(1, [[22, 4, 49, 20, 1]])
    p.add(_im(48, 48), [])
    return p.freeze()


QUERIES = [dict(row=1, ratio=1.25, pos_cls=2, need_crop=True, crop_start=9, order=[1, 0]), dict(row=3, ratio=1.0, pos_cls=1),
           dict(row=2, ratio=0.8, pos_cls=1, need_crop=True, crop_start=4)]
SUPPORTS = [(2, (2, 2, 40, 60)), (1, (53, 5, 54.5, 36))]


def _plan(pool, queries=QUERIES, supports=SUPPORTS, hw=(60, 64)):
    return PL.plan_episode(pool, queries, supports, holder_hw=hw, target_size=48, support_size=32)


# ---- composed_boxes_numpy, by hand ---------------------------------------------------------------------------------------
def _part(boxes, dy, dx, h, w, x_s=0, y_s=0, im_scale=1.0, order=None):
    boxes = None if boxes is None else np.asarray(boxes, dtype=np.float32).reshape(-1, 5)
    return dict(boxes=boxes, order=[] if boxes is None else (list(range(len(boxes))) if order is None else order),
                im_scale=im_scale, x_s=x_s, y_s=y_s, h=h, w=w, dy=dy, dx=dx)


def _kept(out):
    return [r.tolist() for r in out[2][:out[3]]]


def test_composed_boxes_hand_worked():
    """Part 0: the window x [10, 29], y [0, 19] (20 x 20) painted at (dy 5, dx 30), so D_0 = [30, 49] x [5, 24].
         box A (12, 2, 22, 12): u = v = (2, 2, 12, 12), t = (32, 7, 42, 17); full = seen = 100
         box B (0, 0, 20, 10):  u = (-10, 0, 10, 10), v = (0, 0, 10, 10), t = (30, 5, 40, 15); full 200, seen 100
         box C (40, 0, 50, 10): u = (30, 0, 40, 10), v = (19, 0, 19, 10): degenerate whatever the rule
       Part 1: 11 x 6 at (dy 10, dx 37): D_1 = [37, 42] x [10, 20]; its own box (0, 0, 4, 4) -> t = (37, 10, 41, 14).
         hidden(A) = (min(42, 42) - max(32, 37)) * (min(17, 20) - max(7, 10)) = 5 * 7 = 35 -> visible 65 of 100
         hidden(B) = (min(40, 42) - 37) * (min(15, 20) - 10) = 3 * 5 = 15 -> visible 85 of 200 = 0.425"""
    a, b, c = [12, 2, 22, 12, 1], [0, 0, 20, 10, 2], [40, 0, 50, 10, 1]
    parts = [_part([a, b, c], 5, 30, 20, 20, x_s=10), _part([[0, 0, 4, 4, 1]], 10, 37, 11, 6)]
    ta, tb, t1 = [32, 7, 42, 17, 1], [30, 5, 40, 15, 2], [37, 10, 41, 14, 1]
    assert _kept(PL.composed_boxes_numpy(parts, 1, 8)) == [ta, tb, t1]  # no rule: only the degenerate box goes
    assert _kept(PL.composed_boxes_numpy(parts, 1, 8, min_visible=0.4)) == [ta, tb, t1]
    assert _kept(PL.composed_boxes_numpy(parts, 1, 8, min_visible=0.5)) == [ta, t1]      # 85 < 100
    assert _kept(PL.composed_boxes_numpy(parts, 1, 8, min_visible=0.65)) == [ta, t1]     # equality keeps: 65 >= 0.65 * 100
    assert _kept(PL.composed_boxes_numpy(parts, 1, 8, min_visible=0.7)) == [t1]
    fs, n_fs, al, n_al = PL.composed_boxes_numpy(parts, 1, 8, min_visible=0.4)
    assert (n_fs, n_al) == (2, 3) and fs[:2].tolist() == [ta, t1] and not fs[2:].any() and not al[3:].any()
    assert fs.dtype == al.dtype == np.float32 and fs.shape == al.shape == (8, 5)
    # the positive class 2 gets label 1; the cut at max_num_box follows the walk order
    fs, n_fs, al, n_al = PL.composed_boxes_numpy(parts, 2, 2, min_visible=0.4)
    assert (n_fs, n_al) == (1, 2) and fs[0].tolist() == [30, 5, 40, 15, 1] and al.tolist() == [ta, tb]
    # a part's order is followed, and a box may be named twice
    parts[0]["order"] = [1, 0, 1]
    assert _kept(PL.composed_boxes_numpy(parts, 1, 8)) == [tb, ta, tb, t1]
    # swapped painting order: part 1's box now lies under D_0 entirely, part 0's boxes under nothing
    swapped = [parts[1], dict(parts[0], order=[0, 1, 2])]
    assert _kept(PL.composed_boxes_numpy(swapped, 1, 8, min_visible=0.01)) == [ta, tb]
    assert _kept(PL.composed_boxes_numpy(swapped, 1, 8)) == [t1, ta, tb]  # f = 0: no rule, the covered box stays


def test_overlapping_covers_count_twice_and_erase_parts_hide():
    """A 20 x 10 box at t = (0, 0, 20, 10), area 200, under two later parts that both cover x [0, 9] (D = [0, 9] x [0, 19]):
    the union hides 9 * 10 = 90 (visible 0.55), the rule as written sums 180 (visible 0.1)"""
    base = _part([[0, 0, 20, 10, 1]], 0, 0, 30, 30)
    cover = _part(None, 0, 0, 20, 10)
    assert PL.composed_boxes_numpy([base, cover], 1, 4, min_visible=0.5)[3] == 1    # one cover: 110 of 200
    assert PL.composed_boxes_numpy([base, cover, cover], 1, 4, min_visible=0.5)[3] == 0  # summed: 20 of 200
    assert PL.composed_boxes_numpy([base, cover, cover], 1, 4, min_visible=0.1)[3] == 1  # 20 >= 0.1 * 200
    assert PL.composed_boxes_numpy([base, cover, cover], 1, 4, min_visible=0.0)[3] == 1
    # an erase part (no boxes, no source) hides like any other; earlier parts hide nothing
    assert PL.composed_boxes_numpy([cover, base], 1, 4, min_visible=0.9)[3] == 1
    full = _part(None, 0, 0, 11, 21)  # D = [0, 20] x [0, 10]: all of it
    assert PL.composed_boxes_numpy([base, full], 1, 4, min_visible=0.001)[3] == 0
    assert PL.composed_boxes_numpy([base, full], 1, 4)[3] == 1


def test_one_part_at_the_origin_is_episode_boxes_numpy(pool):
    q = dict(row=1, pos_cls=1, crop=(5, 9, 40, 60), order=[1, 0])
    # visible fractions at this window: box 0 0.85 (cut on the left), box 1 0.93 (cut below)
    for f in (None, 0.3, 0.9):
        plain = PL.plan_episode(pool, [dict(q, min_visible=f)], holder_hw=(48, 64), target_size=48)
        comp = PL.plan_episode(pool, [dict(q, min_visible=f, at=(0, 0))], holder_hw=(48, 64), target_size=48)
        assert comp.composed and not plain.composed
        for a, b in zip(plain.boxes_numpy(pool, 4), comp.boxes_numpy(pool, 4)):
            assert np.array_equal(a, b)
    assert plain.boxes_numpy(pool, 4)[3].tolist() == [1]


# ---- helpers -------------------------------------------------------------------------------------------------------------
def test_mosaic_tiles_the_holder_for_every_centre(pool):
    H, W = 12, 10
    rows = [1, 2, 3, 4]  # prepared at 48: 48 x 69, 64 x 48, 48 x 69, 48 x 48: all cover any quadrant of 12 x 10
    for cy in range(1, H):
        for cx in range(1, W):
            q = PL.mosaic_query(pool, rows, (cy, cx), (H, W), target_size=48)
            assert len(q["parts"]) == 4 and [p["row"] for p in q["parts"]] == rows
            count = np.zeros((H, W), dtype=np.int32)
            for p in q["parts"]:
                (dy, dx), (_, _, h, w) = p["at"], p["crop"]
                assert h >= 1 and w >= 1
                count[dy:dy + h, dx:dx + w] += 1
            assert (count == 1).all(), (cy, cx)
            plan = PL.plan_episode(pool, [q], holder_hw=(H, W), target_size=48)
            assert plan.composed and plan.max_parts == 4
    q = PL.mosaic_query(pool, rows, (5, 3), (H, W), target_size=48)
    # the default windows touch the centre with the image's corner: the top-left part ends at its last row and column
    assert [p["crop"] for p in q["parts"]] == [(43, 66, 5, 3), (59, 0, 5, 7), (0, 66, 7, 3), (0, 0, 7, 7)]
    assert q["min_visible"] == 0.5 and q["pos_cls"] == 1
    q = PL.mosaic_query(pool, rows, (5, 3), (H, W), target_size=[48, 24, 48, 48], starts=[(1, 2), None, None, (4, 4)],
                        colors=[None, PL.color_matrix(), None, None], pos_cls=2, min_visible=0.25)
    assert q["parts"][0]["crop"] == (1, 2, 5, 3) and q["parts"][3]["crop"] == (4, 4, 7, 7) and q["parts"][1]["target_size"] == 24
    assert "color" in q["parts"][1] and "color" not in q["parts"][0] and (q["pos_cls"], q["min_visible"]) == (2, 0.25)
    for center in [(0, 3), (5, 0), (12, 3), (5, 10)]:
        with pytest.raises(ValueError, match="leaves no room"):
            PL.mosaic_query(pool, rows, center, (H, W), target_size=48)
    with pytest.raises(ValueError, match="does not cover"):
        PL.mosaic_query(pool, rows, (60, 40), (100, 80), target_size=48)
    with pytest.raises(ValueError, match="four rows"):
        PL.mosaic_query(pool, rows[:3], (5, 3), (H, W))


def test_paste_part_carries_exactly_one_box(pool):
    # row 1 at target 48: scale 48 / 37; box 1 (10, 5, 50, 36) -> x 12.97..64.86, y 6.49..46.70 -> window x [12, 65], y [6, 47]
    part = PL.paste_part(pool, 1, 1, (3, 4), target_size=48)
    assert part == dict(row=1, crop=(6, 12, 42, 54), at=(3, 4), target_size=48, order=[1])
    plan = PL.plan_episode(pool, [dict(parts=[part], pos_cls=2, min_visible=0.5)], holder_hw=(48, 64), target_size=48)
    fs, n_fs, al, n_al = plan.boxes_numpy(pool, 4)
    assert n_al.tolist() == [1] and n_fs.tolist() == [1] and al[0, 0, 4] == 2
    s = 48 / 37.0
    want = np.array([10 * s - 12 + 4, 5 * s - 6 + 3, 50 * s - 12 + 4, 36 * s - 6 + 3])
    assert np.abs(al[0, 0, :4] - want).max() < 1e-4
    # the margin grows the window and stops at the image (48 x 69 prepared)
    assert PL.paste_part(pool, 1, 1, (0, 0), target_size=48, margin=5)["crop"] == (1, 7, 47, 62)
    assert PL.paste_part(pool, 1, 1, (0, 0), target_size=48, margin=100)["crop"] == (0, 0, 48, 69)
    assert "color" in PL.paste_part(pool, 1, 0, (0, 0), color=PL.color_matrix())
    with pytest.raises(ValueError, match="has no box"):
        PL.paste_part(pool, 1, 2, (0, 0))


def test_draw_helpers_take_a_fixed_number_of_draws(pool):
    rows = [1, 2, 3, 4]

    def after(fn, n):
        ga, gb = np.random.default_rng(3), np.random.default_rng(3)
        out = fn(ga)
        gb.random(n)
        assert ga.random() == gb.random()
        return out

    q = after(lambda g: PL.draw_mosaic(g, pool, rows, (40, 44), target_size=48, min_visible=0.3), 10)
    assert len(q["parts"]) == 4 and q["min_visible"] == 0.3
    (cy, cx) = q["parts"][3]["at"]
    assert 10 <= cy <= 30 and 11 <= cx <= 33  # the centre falls in the middle half by default
    PL.plan_episode(pool, [q], holder_hw=(40, 44), target_size=48)  # every window lies inside its prepared image
    assert after(lambda g: PL.draw_mosaic(g, pool, rows, (200, 200), target_size=48), 10) is None  # quadrants too large
    part = after(lambda g: PL.draw_paste(g, pool, 1, 1, (48, 64), target_size=48), 2)
    assert part["crop"] == (6, 12, 42, 54) and 0 <= part["at"][0] <= 6 and 0 <= part["at"][1] <= 10
    assert after(lambda g: PL.draw_paste(g, pool, 1, 1, (40, 64), target_size=48), 2) is None  # 42 rows into 40
    g1, g2 = np.random.default_rng(11), np.random.default_rng(11)
    assert [PL.draw_paste(g1, pool, 1, 0, (48, 64), target_size=48) for _ in range(4)] == \
        [PL.draw_paste(g2, pool, 1, 0, (48, 64), target_size=48) for _ in range(4)]


# ---- the plan's words ----------------------------------------------------------------------------------------------------
def test_plain_and_augmented_plans_have_the_words_they_had(pool):
    want = np.load(GOLDEN)
    plain = _plan(pool)
    assert plain.words.dtype == np.int32 and np.array_equal(plain.words, want)
    assert not plain.composed and plain.c_off is None and plain.max_parts == 0 and not plain.augmented
    m0, m1 = PL.color_matrix(-12, 1.3, 0.6, 17), PL.color_matrix(hue=40)
    aug = _plan(pool, [dict(QUERIES[0], color=m0, min_visible=0.25), QUERIES[1], dict(QUERIES[2], min_visible=0.0)],
                [SUPPORTS[0] + (m1,), SUPPORTS[1]])
    assert aug.augmented and not aug.composed and aug.a_off == 84 and aug.words.size == 84 + 5 * PL.EP_AWORDS
    assert np.array_equal(aug.words[:84], want)
    sec = aug.words[84:].reshape(5, PL.EP_AWORDS)
    assert np.array_equal(sec.view(np.float32)[0, :12].reshape(3, 4), m0) and np.array_equal(sec.view(np.float32)[3, :12].reshape(3, 4), m1)
    assert sec[:, PL.A_FLAGS].tolist() == [PL.A_HAS_COLOR | PL.A_HAS_VISIBLE, 0, 0, PL.A_HAS_COLOR, 0]
    assert np.array_equal(PL._pack_plan(aug.queries, aug.supports, augmented=True), aug.words)


def test_composed_plan_words(pool):
    want = np.load(GOLDEN)
    m = PL.color_matrix(-12, 1.3, 0.6, 17)
    parts = [dict(row=1, crop=(5, 9, 40, 60), at=(0, 0)),
             dict(row=2, crop=(10, 4, 20, 30), at=(30, 34), target_size=36, color=m, order=[0, 0, 0]),
             dict(erase=(7, 8, 5, 6))]
    comp = dict(parts=parts, pos_cls=1, min_visible=0.25)
    plan = _plan(pool, [QUERIES[0], comp, QUERIES[2]])
    plain = _plan(pool, [QUERIES[0], dict(row=1, pos_cls=1, crop=(5, 9, 40, 60), order=[]), QUERIES[2]])
    # the front of the plan is the plain plan in which the composed query is part 0's window with no boxes of its own
    assert plan.composed and not plan.augmented and plan.max_parts == 3 and plan.c_off == plain.words.size + (plain.words.size & 1)
    assert plan.c_off % 2 == 0 and np.array_equal(plan.words[:plain.words.size], plain.words)
    # the other records are the golden plan's; the third one's box order has moved up by the word query 1 no longer takes
    assert np.array_equal(plan.words[:16], want[:16]) and np.array_equal(np.delete(plan.words[32:48], PL.Q_ORDER_OFF),
                                                                         np.delete(want[32:48], PL.Q_ORDER_OFF))
    assert plan.words[32 + PL.Q_ORDER_OFF] == want[32 + PL.Q_ORDER_OFF] - 1
    p_off = plan.c_off + 3 * PL.EP_CWORDS
    o_off = p_off + 3 * 3 * PL.EP_PWORDS
    assert plan.words.size == o_off + 2 + 0 + 3  # part 0's two boxes as stored, the erase part's none, the named three
    heads = plan.words[plan.c_off:p_off].reshape(3, PL.EP_CWORDS)
    assert heads[:, PL.C_NPARTS].tolist() == [1, 3, 1] and heads[:, PL.C_CLS].tolist() == [2, 1, 1]
    assert heads[:, PL.C_FLAGS].tolist() == [0, PL.A_HAS_VISIBLE, 0]
    assert heads.view(np.float32)[:, PL.C_MIN_VISIBLE].tolist() == [0, 0.25, 0] and not heads[:, 4:].any()
    recs = plan.words[p_off:o_off].reshape(3, 3, PL.EP_PWORDS)
    assert not recs[0, 1:].any() and not recs[2, 1:].any()  # unused records of the shorter tables
    # a query that is not composed: its own record with a destination of (0, 0), its order where it always was
    for b in (0, 2):
        q, r = plan.words[b * 16:(b + 1) * 16], recs[b, 0]
        assert np.array_equal(r[:12], q[:12]) and r[PL.P_DY] == r[PL.P_DX] == 0 and r[PL.P_ORDER_OFF] == q[PL.Q_ORDER_OFF]
        assert r[PL.P_FLAGS] == 0 and np.array_equal(r[PL.P_M:PL.P_M + 12].view(np.float32).reshape(3, 4), np.eye(3, 4))
    r = recs[1]
    assert r[:, PL.P_ROW].tolist() == [1, 2, -1] and r[:, PL.P_NORDER].tolist() == [2, 3, 0]
    assert r[:, PL.P_YS:PL.P_DX + 1].tolist() == [[5, 9, 40, 60, 59, 39, 0, 0], [10, 4, 20, 30, 29, 19, 30, 34], [0, 0, 5, 6, 5, 4, 7, 8]]
    assert r[:, PL.P_ORDER_OFF].tolist() == [o_off, o_off + 2, o_off + 5] and r[:, PL.P_FLAGS].tolist() == [0, PL.A_HAS_COLOR, 0]
    assert plan.words[o_off:].tolist() == [0, 1, 0, 0, 0]
    scales = np.ascontiguousarray(r[:, PL.P_SCALE:PL.P_SCALE + 4]).view(np.float64)
    assert scales.tolist() == [[48 / 37.0, 1 / (48 / 37.0)], [36 / 48.0, 1 / (36 / 48.0)], [1.0, 1.0]]
    assert np.array_equal(r[1, PL.P_M:PL.P_M + 12].view(np.float32).reshape(3, 4), m)
    assert r[:, PL.P_OH:PL.P_OW + 1].tolist() == [[48, 69], [48, 36], [5, 6]]
    # the host records
    host = plan.queries[1]
    assert [p["erase"] for p in host["parts"]] == [False, False, True] and host["im_scale"] == 48 / 37.0 and host["min_visible"] == 0.25
    assert (host["parts"][1]["dy"], host["parts"][1]["dx"], host["parts"][1]["h"], host["parts"][1]["w"]) == (30, 34, 20, 30)
    assert "parts" not in plan.queries[0]
    # a support's colour map still makes the augmentation section, in front of the composed one; an odd end is padded
    both = _plan(pool, [comp], [SUPPORTS[0] + (m,)])
    assert both.composed and both.augmented and both.a_off == 32 and both.c_off == 32 + 2 * PL.EP_AWORDS
    odd = _plan(pool, [dict(row=0, ratio=1.0, pos_cls=2), dict(row=4, pos_cls=1, crop=(0, 0, 48, 48), at=(0, 0))], [])
    assert odd.c_off == 34 and odd.words[33] == 0 and odd.words[32] == 0 and odd.max_parts == 1
    # min_visible or color on a query of a composed plan travel in the composed section: no augmentation section
    mixed = _plan(pool, [dict(QUERIES[1], color=m, min_visible=0.5), dict(row=4, pos_cls=1, crop=(0, 0, 48, 48), at=(0, 0))], [])
    assert mixed.composed and not mixed.augmented
    rec = mixed.words[mixed.c_off + 2 * PL.EP_CWORDS:][:PL.EP_PWORDS]
    assert rec[PL.P_FLAGS] == PL.A_HAS_COLOR and np.array_equal(rec[PL.P_M:PL.P_M + 12].view(np.float32).reshape(3, 4), m)
    assert mixed.words[mixed.c_off + PL.C_FLAGS] == PL.A_HAS_VISIBLE


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_entry_points_check_the_section_without_a_gpu():
    """the argument checks come before any launch and before the pointers are looked at (all null here, so a call that
    passed every other check still ends at "null pointer"); tests/test_gpu_episode_compose.py repeats them with real buffers"""
    from dana_amd import _lib
    L = _lib.lib()
    # plan_words, c_off, max_parts for batch 2: the section takes 2 * 8 + 2 * max_parts * 32 words behind c_off
    cases = [((100 + 16 + 64 * 4, 100, 4), "null pointer"),
             ((100 + 16 + 64 * 4 - 1, 100, 4), "does not fit the plan"),
             ((100 + 16 + 64 * 4, 100, 5), "does not fit the plan"),
             ((1000, 101, 4), "odd word"),
             ((1000, -2, 4), "odd word"),
             ((1000, 100, 0), r"part count outside 1\.\.16"),
             ((100000, 100, 17), r"part count outside 1\.\.16"),
             ((100 + 16 + 64 * 16, 100, 16), "null pointer")]
    for (n_words, c_off, max_parts), message in cases:
        with pytest.raises(_lib.DanaError, match="dana_episode_queries_composed: .*" + message):
            L.call("dana_episode_queries_composed", None, 64, None, None, 1, None, n_words, c_off, max_parts, 2, None, None, 8, 8,
                   None, None)
        with pytest.raises(_lib.DanaError, match="dana_episode_boxes_composed: .*" + message):
            L.call("dana_episode_boxes_composed", None, 0, None, 1, None, n_words, c_off, max_parts, 2, 4, None, None, None, None,
                   None)
    with pytest.raises(_lib.DanaError, match="bad shape"):
        L.call("dana_episode_queries_composed", None, 64, None, None, 1, None, 1000, 100, 4, 0, None, None, 8, 8, None, None)


def test_refusals(pool):
    class _Dev:  # stands for a device tensor where there is no device: the check reads `is_cuda`
        is_cuda = True
    ok = dict(row=1, crop=(5, 9, 40, 60), at=(0, 0))
    one = dict(erase=(0, 0, 1, 1))
    bad = [(dict(parts=[one] * 17, pos_cls=1), "1 to 16 parts, got 17"),
           (dict(parts=[], pos_cls=1), "1 to 16 parts, got 0"),
           (dict(parts=[dict(row=1, at=(0, 0))], pos_cls=1), "part 0 needs row, crop and at"),
           (dict(parts=[ok, dict(row=1, crop=(0, 0, 4, 4))], pos_cls=1), "part 1 needs row, crop and at"),
           (dict(parts=[dict(crop=(0, 0, 4, 4), at=(0, 0))], pos_cls=1), "part 0 needs row, crop and at"),
           (dict(row=1, at=(0, 0), pos_cls=1), "part 0 needs row, crop and at"),
           (dict(parts=[dict(ok, at=(9, 0))], pos_cls=1), r"part 0's destination \(y 9, x 0, 40 x 60\) leaves the holder"),
           (dict(parts=[dict(ok, at=(0, 5))], pos_cls=1), "leaves the holder"),
           (dict(parts=[dict(ok, at=(-1, 0))], pos_cls=1), "leaves the holder"),
           (dict(parts=[ok, dict(erase=(40, 60, 9, 4))], pos_cls=1), "part 1's destination"),
           (dict(parts=[dict(erase=(0, 0, 0, 4))], pos_cls=1), "leaves the holder"),
           (dict(parts=[dict(ok, flip=True)], pos_cls=1), "unknown key 'flip' in part 0"),
           (dict(parts=[dict(ok, min_visible=0.5)], pos_cls=1), "unknown key 'min_visible' in part 0"),
           (dict(parts=[dict(ok, pos_cls=1)], pos_cls=1), "unknown key 'pos_cls' in part 0"),
           (dict(parts=[dict(erase=(0, 0, 4, 4), row=1)], pos_cls=1), "erase together with row"),
           (dict(parts=[dict(ok, erase=(0, 0, 4, 4))], pos_cls=1), "erase together with row, crop, at"),
           (dict(parts=[dict(erase=(0, 0, 4))], pos_cls=1), "erase must have 4 entries"),
           (dict(parts=[dict(ok, at=(0, 0, 0))], pos_cls=1), "at must have 2 entries"),
           (dict(parts=[dict(ok, at=_Dev())], pos_cls=1), "at is a device tensor"),
           (dict(parts=[dict(erase=_Dev())], pos_cls=1), "erase is a device tensor"),
           (dict(parts=[dict(ok, crop=_Dev())], pos_cls=1), "crop is a device tensor"),
           (dict(parts=[dict(ok, row=_Dev())], pos_cls=1), "row is a device tensor"),
           (dict(parts=[dict(ok, color=_Dev())], pos_cls=1), "color is a device tensor"),
           (dict(parts=[dict(ok, order=_Dev())], pos_cls=1), "order is a device tensor"),
           (dict(parts=[dict(ok, target_size=_Dev())], pos_cls=1), "target_size is a device tensor"),
           (dict(parts=_Dev(), pos_cls=1), "parts is a device tensor"),
           (dict(parts=[ok], pos_cls=_Dev()), "pos_cls is a device tensor"),
           (dict(parts=[ok], pos_cls=1, min_visible=_Dev()), "min_visible is a device tensor"),
           (dict(parts=[ok], pos_cls=1, min_visible=1.5), r"min_visible of a composed query must lie in \[0, 1\]"),
           (dict(parts=[ok], pos_cls=1, ratio=1.0), "cannot carry ratio"),
           (dict(ok, pos_cls=1, need_crop=True), "cannot carry need_crop"),
           (dict(ok, pos_cls=1, crop_start=3), "cannot carry crop_start"),
           (dict(parts=[ok], pos_cls=1, row=1), "a query with parts cannot carry row"),
           (dict(parts=[ok], pos_cls=1, color=np.eye(3, 4)), "a query with parts cannot carry color"),
           (dict(parts=[ok], pos_cls=1, at=(0, 0)), "a query with parts cannot carry at"),
           (dict(parts=[dict(ok, crop=(0, 10, 48, 60))], pos_cls=1), "leaves the prepared image"),
           (dict(parts=[dict(ok, color=np.eye(3))], pos_cls=1), r"color must be a \[3\]\[4\] matrix"),
           (dict(parts=[dict(ok, order=[2])], pos_cls=1), "names a box outside")]
    for q, message in bad:
        with pytest.raises(ValueError, match=message):
            PL.plan_episode(pool, [q], holder_hw=(48, 64), target_size=48)
    # None is the same as leaving the key out, in a query and in a part
    plan = PL.plan_episode(pool, [dict(row=1, ratio=1.0, pos_cls=1, at=None, parts=None)], holder_hw=(48, 64), target_size=48)
    assert not plan.composed
    plan = PL.plan_episode(pool, [dict(parts=[dict(ok, erase=None, color=None, order=None, target_size=None)], pos_cls=1,
                                       ratio=None, need_crop=False)], holder_hw=(48, 64), target_size=48)
    assert plan.composed and plan.max_parts == 1
    # sixteen parts are fine
    assert PL.plan_episode(pool, [dict(parts=[one] * 16, pos_cls=1)], holder_hw=(48, 64), target_size=48).max_parts == 16
