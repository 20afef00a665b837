"""Host side of training-time augmentation in the episode assembler (dana_amd/pipeline.py): color_matrix on hand-worked
answers, draw_color_matrix under seeds, the plan's words with and without augmentation keys (the words of a plain plan are
pinned by tests/golden/episode_plan_words.npy, written before the feature existed), the visibility rule of
episode_boxes_numpy on four boxes, and every refusal. No device."""
import os

import numpy as np
import pytest

from dana_amd import pipeline as PL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "episode_plan_words.npy")
IDENTITY = np.eye(3, 4, dtype=np.float32)
LUMA = np.array([0.299, 0.587, 0.114])


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


# the plan whose words the fixture holds
QUERIES = [dict(row=1, ratio=1.25, pos_cls=2, need_crop=True, crop_start=9, order=[1, 0]), dict(row=3, ratio=1.0, pos_cls=1),
           dict(row=2, ratio=0.8, pos_cls=1, need_crop=True, crop_start=4)]
SUPPORTS = [(2, (2, 2, 40, 60)), (1, (53, 5, 54.5, 36))]


def _plan(pool, queries=QUERIES, supports=SUPPORTS):
    return PL.plan_episode(pool, queries, supports, holder_hw=(60, 64), target_size=48, support_size=32)


# ---- color_matrix ------------------------------------------------------------------------------------------------------
def test_color_matrix_hand_worked():
    m = PL.color_matrix()
    assert m.dtype == np.float32 and m.shape == (3, 4) and m.flags["C_CONTIGUOUS"] and np.array_equal(m, IDENTITY)
    # saturation 0: every channel becomes the luma
    assert np.array_equal(PL.color_matrix(saturation=0.0), np.tile(np.append(LUMA, 0.0), (3, 1)).astype(np.float32))
    # contrast 0: everything collapses onto the pivot
    want = np.zeros((3, 4), dtype=np.float32)
    want[:, 3] = 128.0
    assert np.array_equal(PL.color_matrix(contrast=0.0), want)
    want[:, 3] = 100.0
    assert np.array_equal(PL.color_matrix(contrast=0.0, pivot=100.0), want)
    # a full turn of the hue is the identity again (cos / sin of 2 pi in double, then one float32 rounding)
    assert np.abs(PL.color_matrix(hue=360.0) - IDENTITY).max() <= 2 ** -23
    # half a turn keeps the luma of every pixel: luma . M[:, :3] == luma
    h180 = PL.color_matrix(hue=180.0).astype(np.float64)
    assert np.abs(LUMA @ h180[:, :3] - LUMA).max() < 1e-6 and np.abs(h180[:, :3] - np.eye(3)).max() > 0.5
    # brightness alone: only column 3
    b = PL.color_matrix(brightness=-20.0)
    assert np.array_equal(b[:, :3], np.eye(3, dtype=np.float32)) and b[:, 3].tolist() == [-20.0, -20.0, -20.0]
    # the order is brightness, then contrast: 2 * ((v + 10) - 128) + 128 = 2 v - 108, not 2 v - 118
    bc = PL.color_matrix(brightness=10.0, contrast=2.0)
    assert np.array_equal(bc[:, :3], 2 * np.eye(3, dtype=np.float32)) and bc[:, 3].tolist() == [-108.0, -108.0, -108.0]
    # saturation after contrast: the rows still sum to the contrast (luma weights sum to 1)
    cs = PL.color_matrix(contrast=1.5, saturation=0.25).astype(np.float64)
    assert np.abs(cs[:, :3].sum(1) - 1.5).max() < 1e-6 and np.abs(cs[:, 3] + 64.0).max() < 1e-5


def test_apply_color_numpy_is_the_tap_expression():
    im = np.array([[[10, 200, 30], [255, 0, 128]]], dtype=np.uint8)
    assert np.array_equal(PL.apply_color_numpy(im, IDENTITY), im.astype(np.float32))
    swap = np.array([[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0]], dtype=np.float32)
    assert np.array_equal(PL.apply_color_numpy(im, swap), im[..., ::-1].astype(np.float32))
    up = IDENTITY.copy()
    up[:, 3] = 40
    assert PL.apply_color_numpy(im, up).tolist() == [[[50, 240, 70], [255, 40, 168]]]  # saturates at 255
    m = PL.color_matrix(-12, 1.3, 0.6, 17)
    r, g, b = [np.float32(v) for v in im[0, 0]]
    want = [min(max(((m[j, 0] * r + m[j, 1] * g) + m[j, 2] * b) + m[j, 3], np.float32(0)), np.float32(255)) for j in range(3)]
    got = PL.apply_color_numpy(im, m)
    assert got.dtype == np.float32 and got[0, 0].tolist() == [float(v) for v in want]


def test_draw_color_matrix_seeds_and_ranges():
    a = [PL.draw_color_matrix(np.random.default_rng(7)) for _ in range(2)]
    assert np.array_equal(a[0], a[1]) and a[0].dtype == np.float32 and a[0].shape == (3, 4)
    g1, g2 = np.random.default_rng(11), np.random.default_rng(11)
    seq1, seq2 = [PL.draw_color_matrix(g1) for _ in range(8)], [PL.draw_color_matrix(g2) for _ in range(8)]
    assert all(np.array_equal(x, y) for x, y in zip(seq1, seq2))
    assert any(not np.array_equal(x, IDENTITY) for x in seq1) and not all(np.array_equal(x, seq1[0]) for x in seq1)
    assert np.array_equal(PL.draw_color_matrix(np.random.default_rng(7), p=0.0), IDENTITY)
    g = np.random.default_rng(5)
    seen = {k: 0 for k in ("brightness", "contrast", "saturation", "hue")}
    for _ in range(200):
        d = PL.draw_color_params(g, brightness=20, contrast=(0.7, 1.2), saturation=(0.4, 1.1), hue=9, p=1.0)
        assert -20 <= d["brightness"] <= 20 and 0.7 <= d["contrast"] <= 1.2 and 0.4 <= d["saturation"] <= 1.1
        assert -9 <= d["hue"] <= 9
        for k, neutral in (("brightness", 0.0), ("contrast", 1.0), ("saturation", 1.0), ("hue", 0.0)):
            seen[k] += d[k] != neutral
    assert all(n == 200 for n in seen.values())  # p = 1 applies every component
    # the draw and the matrix agree, and a draw always takes eight numbers from the stream
    ga, gb = np.random.default_rng(3), np.random.default_rng(3)
    assert np.array_equal(PL.color_matrix(**PL.draw_color_params(ga)), PL.draw_color_matrix(gb))
    gc = np.random.default_rng(3)
    gc.random(8)
    assert ga.random() == gc.random()


# ---- the plan's words ----------------------------------------------------------------------------------------------------
def test_plain_plan_has_the_words_it_always_had(pool):
    plan = _plan(pool)
    want = np.load(GOLDEN)
    assert want.dtype == np.int32 and plan.words.dtype == np.int32 and np.array_equal(plan.words, want)
    assert plan.augmented is False and plan.a_off is None
    # geometry keys alone need no section: the records differ, the plan stays a plain one
    geo = _plan(pool, [dict(QUERIES[0], target_size=40, crop_start=2), dict(row=3, pos_cls=1, crop=(2, 3, 20, 30)), QUERIES[2]])
    assert geo.augmented is False and geo.words.size == want.size


def test_augmented_plan_carries_the_section(pool):
    m0, m1 = PL.color_matrix(-12, 1.3, 0.6, 17), PL.color_matrix(hue=40)
    queries = [dict(QUERIES[0], color=m0, min_visible=0.25), QUERIES[1], dict(QUERIES[2], min_visible=0.0)]
    plan = _plan(pool, queries, [SUPPORTS[0] + (m1,), SUPPORTS[1]])
    plain = np.load(GOLDEN)
    # 3 * 16 + 2 * 16 + 4 order words = 84 (even): the section follows at once; with one more order word it moves to 86
    assert plan.augmented and plan.a_off == 84 and plan.a_off % 2 == 0 and plan.words.size == 84 + 5 * PL.EP_AWORDS
    assert np.array_equal(plan.words[:84], plain)  # nothing in front of the section changes
    sec = plan.words[84:].reshape(5, PL.EP_AWORDS)
    f32 = sec.view(np.float32)
    assert np.array_equal(f32[0, :12].reshape(3, 4), m0) and f32[0, PL.A_MIN_VISIBLE] == np.float32(0.25)
    assert sec[:, PL.A_FLAGS].tolist() == [PL.A_HAS_COLOR | PL.A_HAS_VISIBLE, 0, 0, PL.A_HAS_COLOR, 0]
    for k in (1, 2, 4):  # no map: the identity, and no flag
        assert np.array_equal(f32[k, :12].reshape(3, 4), IDENTITY) and f32[k, PL.A_MIN_VISIBLE] == 0
    assert np.array_equal(f32[3, :12].reshape(3, 4), m1)
    assert not sec[:, 14:].any()
    assert plan.queries[0]["min_visible"] == 0.25 and np.array_equal(plan.supports[0]["color"], m1)
    odd = _plan(pool, [dict(row=0, ratio=1.0, pos_cls=2, color=m0)], [])
    assert odd.words.size - 1 * PL.EP_AWORDS == 18 and odd.a_off == 18 and odd.words[17] == 0  # 16 + 1 order word, padded
    # supports only (what support_crops takes)
    sup = PL.plan_episode(pool, (), [SUPPORTS[0] + (m1,)], target_size=48, support_size=32)
    assert sup.augmented and sup.a_off == 16 and np.array_equal(sup.words[16:28].view(np.float32).reshape(3, 4), m1)


def test_min_visible_and_flags_survive_pack_plan(pool):
    plan = _plan(pool, [dict(QUERIES[0], min_visible=0.4), dict(QUERIES[1], color=PL.color_matrix())], [])
    again = PL._pack_plan(plan.queries, plan.supports, augmented=True)
    assert np.array_equal(again, plan.words)
    a = plan.a_off
    assert plan.words[a + PL.A_MIN_VISIBLE:a + PL.A_MIN_VISIBLE + 1].view(np.float32)[0] == np.float32(0.4)
    assert plan.words[a + PL.A_FLAGS] == PL.A_HAS_VISIBLE and plan.words[a + PL.EP_AWORDS + PL.A_FLAGS] == PL.A_HAS_COLOR
    plain = PL._pack_plan(plan.queries, plan.supports)  # the plain form of the same records: no section, no padding word
    assert plain.size == 35 and a == 36 and np.array_equal(plain, plan.words[:35]) and plan.words[35] == 0


def test_per_query_scale_and_crop_records(pool):
    qs = _plan(pool, [dict(row=1, ratio=1.0, pos_cls=1, target_size=32), dict(row=1, ratio=1.0, pos_cls=1)], []).queries
    ref = PL.plan_episode(pool, [dict(row=1, ratio=1.0, pos_cls=1)], holder_hw=(60, 64), target_size=32).queries[0]
    assert all(np.array_equal(qs[0][k], ref[k]) for k in ref) and qs[0]["im_scale"] == 32.0 / 37.0 and qs[1]["im_scale"] == 48.0 / 37.0
    # a free window of the 48 x 69 prepared image of row 1: start, copy window, clamps at w - 1 and h - 1
    q = _plan(pool, [dict(row=1, pos_cls=1, crop=(5, 9, 40, 60))], []).queries[0]
    assert (q["y_s"], q["x_s"], q["copy_h"], q["copy_w"], q["clamp_x"], q["clamp_y"]) == (5, 9, 40, 60, 59, 39)
    # a window larger than the holder is copied as far as the holder goes; the clamps keep the window's size
    q = PL.plan_episode(pool, [dict(row=1, pos_cls=1, crop=(0, 0, 48, 69))], holder_hw=(40, 64), target_size=48).queries[0]
    assert (q["copy_h"], q["copy_w"], q["clamp_x"], q["clamp_y"]) == (40, 64, 68, 47)
    with pytest.raises(ValueError, match="larger than the holder"):  # 64x48 at 60 -> 80 x 60 into 60 x 64
        _plan(pool, [dict(row=2, ratio=0.75, pos_cls=1, target_size=60)], [])
    # the holder for rows 1, 2 drawn at 32 or 48: prepared 48 x 69 and 64 x 48; at ratio 1 only the squares
    assert PL.scales_holder_hw(pool, [1, 2], (32, 48)) == (64, 69)
    assert PL.scales_holder_hw(pool, [1, 2], (32, 48), ratios=[1.0, 1.0]) == (48, 48)
    assert PL.scales_holder_hw(pool, [1, 2], (32, 48), ratios=[1.4, 0.75]) == (64, 69)


# ---- visibility ------------------------------------------------------------------------------------------------------------
def test_visibility_on_four_boxes():
    """x window [20, 49] (x_s 20, clamp 29), y untouched. full areas and what the clamp leaves:
       box 0 (25, 0, 45, 10): inside -> 20 * 10 of 20 * 10 = 1
       box 1 (10, 0, 30, 10): u = (-10, 10) -> v = (0, 10): 10 * 10 of 20 * 10 = 0.5
       box 2 (40, 0, 60, 8):  u = (20, 40) -> v = (20, 29): 9 * 8 of 20 * 8 = 0.45
       box 3 (60, 0, 70, 10): right of the window: degenerate whatever f is"""
    boxes = np.array([[25, 0, 45, 10, 1], [10, 0, 30, 10, 1], [40, 0, 60, 8, 2], [60, 0, 70, 10, 1]], dtype=np.float32)
    args = (boxes, [0, 1, 2, 3], 1.0, 20, 0, 29, -1, 1, 4)
    kept = lambda f: [r[:4].tolist() for r in PL.episode_boxes_numpy(*args, min_visible=f)[2] if r.any()]
    b0, b1, b2 = [5, 0, 25, 10], [0, 0, 10, 10], [20, 0, 29, 8]
    assert kept(0.0) == [b0, b1, b2] == [r[:4].tolist() for r in PL.episode_boxes_numpy(*args)[2] if r.any()]
    assert kept(0.4) == [b0, b1, b2] and kept(0.47) == [b0, b1]
    assert kept(0.5) == [b0, b1] and kept(0.6) == [b0] and kept(1.0) == [b0]  # equality keeps: 100 >= 0.5 * 200
    fs, n_fs, al, n_al = PL.episode_boxes_numpy(*args, min_visible=0.6)
    assert (n_fs, n_al) == (1, 1) and fs[0].tolist() == [5, 0, 25, 10, 1] and not fs[1:].any() and not al[1:].any()
    # the positive-class list and the all-class list drop the same boxes
    fs, n_fs, al, n_al = PL.episode_boxes_numpy(*args[:7], 2, 4, min_visible=0.47)
    assert (n_fs, n_al) == (0, 2)


def test_plan_boxes_numpy_passes_min_visible(pool):
    # row 1 at target 48 (scale 48/37), window x in [30, 59], y whole: box 0 (3, 4, 30, 20) -> x (3.9, 38.9) - 30 -> clamped
    # to (0, 8.9): 8.9 of 35.0 = 0.25; box 1 (10, 5, 50, 36) -> x (13.0, 64.9) - 30 -> (0, 29): 29 of 51.9 = 0.56
    q = dict(row=1, pos_cls=1, crop=(0, 30, 48, 30))
    assert PL.plan_episode(pool, [q], holder_hw=(48, 64), target_size=48).boxes_numpy(pool, 4)[3].tolist() == [2]
    assert PL.plan_episode(pool, [dict(q, min_visible=0.3)], holder_hw=(48, 64), target_size=48).boxes_numpy(pool, 4)[3].tolist() == [1]
    assert PL.plan_episode(pool, [dict(q, min_visible=0.6)], holder_hw=(48, 64), target_size=48).boxes_numpy(pool, 4)[3].tolist() == [0]


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(pool):
    class _Dev:  # stands for a device tensor where there is no device: the check reads `is_cuda`
        is_cuda = True
    ok = dict(row=1, ratio=1.0, pos_cls=1)
    bad = [(dict(ok, colour=IDENTITY), "unknown key 'colour'"),
           (dict(ok, flip=True), "unknown key 'flip'"),
           (dict(ok, color=np.eye(3)), r"color must be a \[3\]\[4\] matrix"),
           (dict(ok, color=np.zeros((4, 3))), r"color must be a \[3\]\[4\] matrix"),
           (dict(ok, color=np.full((3, 4), np.nan)), "color is not finite"),
           (dict(ok, color=np.full((3, 4), np.inf)), "color is not finite"),
           (dict(ok, color=np.full((3, 4), 1e39)), "color is not finite"),  # finite in double, not in float32
           (dict(ok, min_visible=-0.1), r"min_visible of row 1 must lie in \[0, 1\]"),
           (dict(ok, min_visible=1.5), r"min_visible of row 1 must lie in \[0, 1\]"),
           (dict(ok, min_visible=float("nan")), r"min_visible of row 1 must lie in \[0, 1\]"),
           (dict(ok, color=_Dev()), "color is a device tensor"),
           (dict(ok, min_visible=_Dev()), "min_visible is a device tensor"),
           (dict(ok, target_size=_Dev()), "target_size is a device tensor"),
           (dict(ok, crop=_Dev()), "crop is a device tensor"),
           (dict(ok, target_size=0), "target_size of row 1 must be positive"),
           (dict(ok, crop=(0, 0, 48, 48), need_crop=True, crop_start=0), "both crop and need_crop"),
           (dict(ok, crop=(0, 0, 48, 48), crop_start=3), "both crop and need_crop"),
           (dict(ok, crop=(0, 10, 48, 60)), "leaves the prepared image"),  # 10 + 60 > 69
           (dict(ok, crop=(-1, 0, 20, 20)), "leaves the prepared image"),
           (dict(ok, crop=(0, 0, 0, 20)), "leaves the prepared image"),
           (dict(ok, crop=(0, 0, 20)), r"crop must be \(y, x, h, w\)")]
    for q, message in bad:
        with pytest.raises(ValueError, match=message):
            PL.plan_episode(pool, [q], holder_hw=(48, 64), target_size=48)
    sup = (1, (3, 4, 30, 20))
    for s, message in [(sup + (np.eye(4),), r"color must be a \[3\]\[4\] matrix"), (sup + (_Dev(),), "color is a device tensor"),
                       (sup + (np.full((3, 4), -np.inf),), "color is not finite"), (sup + (IDENTITY, 1), "a support is")]:
        with pytest.raises(ValueError, match=message):
            PL.plan_episode(pool, (), [s], target_size=48)
    # None is the same as leaving the key out
    plan = PL.plan_episode(pool, [dict(ok, color=None, min_visible=None, crop=None, target_size=None)], [sup + (None,)],
                           holder_hw=(48, 64), target_size=48)
    assert not plan.augmented
