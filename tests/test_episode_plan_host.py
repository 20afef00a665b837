"""Host side of the episode assembler (dana_amd/pipeline.py): ImagePool tables, plan_episode on hand-worked cases, and
episode_boxes_numpy (the numpy restatement of fs_loader.py:183-315 the device kernel is checked against). No device."""
import numpy as np
import pytest
import torch

from dana_amd import pipeline as PL


def _im(h, w):
    return np.zeros((h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def pool():
    p = PL.ImagePool()
    p.add(_im(5, 7), [[1, 1, 4, 3, 2]])                           # row 0
    p.add(_im(37, 53), [[3, 4, 30, 20, 1], [10, 5, 50, 36, 2]])   # row 1
    p.add(_im(64, 48), [[2, 2, 40, 60, 1]])                       # row 2
    p.add_flipped(1, [[22, 4, 49, 20, 1]])                        # row 3: row 1 mirrored (x -> 52 - x)
    p.add(_im(48, 48), [])                                        # row 4
    return p.freeze()


# ---- test 3: ImagePool tables ----------------------------------------------------------------------------------------
def test_pool_tables(pool):
    assert len(pool) == 5 and pool.frozen
    # 5*7*3 = 105 -> 112; 37*53*3 = 5883 -> 112 + 5888 = 6000; 64*48*3 = 9216 -> 15216; 48*48*3 = 6912 -> 22128
    assert pool.offsets.dtype == np.int64 and pool.offsets.tolist() == [0, 112, 6000, 112, 15216]
    assert (pool.offsets % 16 == 0).all() and pool.nbytes == 22128
    assert pool.offsets[3] == pool.offsets[1]  # the flipped twin shares its pixels
    assert pool.meta.dtype == np.int32
    assert pool.meta.tolist() == [[5, 7, 0, 0, 1], [37, 53, 0, 1, 2], [64, 48, 0, 3, 1], [37, 53, 1, 4, 1], [48, 48, 0, 5, 0]]
    assert pool.boxes.dtype == np.float32 and pool.boxes.shape == (5, 5)
    assert pool.boxes[4].tolist() == [22, 4, 49, 20, 1]
    with pytest.raises(RuntimeError, match="frozen"):
        pool.add(_im(4, 4), [])
    with pytest.raises(RuntimeError, match="frozen"):
        pool.add_flipped(0, [])


def test_pool_refuses_what_is_no_image():
    p = PL.ImagePool()
    with pytest.raises(ValueError):
        p.add(np.zeros((4, 4, 3), dtype=np.float32), [])
    with pytest.raises(ValueError):
        p.add(np.zeros((4, 4), dtype=np.uint8), [])
    with pytest.raises(IndexError):
        p.add_flipped(0, [])
    with pytest.raises(RuntimeError, match="freeze"):
        p.add(_im(4, 4), [])
        PL.plan_episode(p, [dict(row=0, ratio=1.0, pos_cls=1)], holder_hw=(8, 8), target_size=4)


# ---- test 1: plan_episode ----------------------------------------------------------------------------------------------
def _q(pool, q, hw, target=48):
    return PL.plan_episode(pool, [q], holder_hw=hw, target_size=target).queries[0]


def test_plan_query_ratio_branches(pool):
    # ratio < 1 (pad_plan pads the height): 64x48 at target 48 is scale 1; ceil(48 / 0.75) = 64 rows
    q = _q(pool, dict(row=2, ratio=0.75, pos_cls=1), (64, 48))
    assert (q["im_scale"], q["oh"], q["ow"]) == (1.0, 64, 48)
    assert (q["y_s"], q["x_s"], q["copy_h"], q["copy_w"], q["out_h"], q["out_w"]) == (0, 0, 64, 48, 64, 48)
    assert (q["clamp_x"], q["clamp_y"]) == (-1, -1) and q["order"].tolist() == [0]
    # ratio > 1 (pads the width): 37x53 at 48 -> scale 48/37, ow = round(68.76) = 69; ceil(48 * 1.5) = 72 columns
    q = _q(pool, dict(row=1, ratio=1.5, pos_cls=2, order=[1, 0]), (48, 72))
    assert q["im_scale"] == 48.0 / 37.0 and (q["oh"], q["ow"]) == (48, 69)
    assert (q["copy_h"], q["copy_w"], q["out_h"], q["out_w"]) == (48, 69, 48, 72)
    assert (q["clamp_x"], q["clamp_y"], q["pos_cls"]) == (-1, -1, 2) and q["order"].tolist() == [1, 0]
    # ratio == 1: the top-left min(h, w) square, every coordinate clamped to [0, trim] (not trim - 1)
    q = _q(pool, dict(row=1, ratio=1.0, pos_cls=1), (48, 64))
    assert (q["copy_h"], q["copy_w"], q["out_h"], q["out_w"]) == (48, 48, 48, 48)
    assert (q["clamp_x"], q["clamp_y"]) == (48, 48)


def test_plan_query_need_crop_and_flipped_row(pool):
    # ratio 1.25 > 1: crop the width to ceil(48 * 1.25) = 60 of 69 columns, from the drawn start; x clamps to [0, 59]
    q = _q(pool, dict(row=1, ratio=1.25, pos_cls=1, need_crop=True, crop_start=9), (48, 64))
    assert (q["y_s"], q["x_s"], q["copy_h"], q["copy_w"]) == (0, 9, 48, 60)  # 9 + 60 = 69: ends at the last column
    assert (q["clamp_x"], q["clamp_y"]) == (59, -1)
    # ratio 0.8 < 1 on 64x48: crop the height to floor(48 / 0.8) = 60 of 64 rows; y clamps to [0, 59]
    q = _q(pool, dict(row=2, ratio=0.8, pos_cls=1, need_crop=True, crop_start=4), (60, 48))
    assert (q["y_s"], q["x_s"], q["copy_h"], q["copy_w"]) == (4, 0, 60, 48)
    assert (q["clamp_x"], q["clamp_y"]) == (-1, 59)
    # a trim larger than the image is cut to it (fs_loader.py:192-193)
    q = _q(pool, dict(row=2, ratio=0.6, pos_cls=1, need_crop=True, crop_start=0), (80, 48))
    assert (q["copy_h"], q["out_h"], q["clamp_y"]) == (64, 80, 63)
    # a flipped row plans like its twin and carries its own boxes
    f, t = _q(pool, dict(row=3, ratio=1.5, pos_cls=1), (48, 72)), _q(pool, dict(row=1, ratio=1.5, pos_cls=1), (48, 72))
    assert {k: f[k] for k in f if k not in ("row", "order")} == {k: t[k] for k in t if k not in ("row", "order")}
    assert f["row"] == 3 and f["order"].tolist() == [0] and t["order"].tolist() == [0, 1]


def test_plan_words_are_the_records(pool):
    plan = PL.plan_episode(pool, [dict(row=1, ratio=1.25, pos_cls=2, need_crop=True, crop_start=9, order=[1, 0]),
                                  dict(row=4, ratio=1.25, pos_cls=1)],
                           [(2, (2, 2, 40, 60))], holder_hw=(48, 64), target_size=48, support_size=32)
    w = plan.words
    assert w.dtype == np.int32 and w.flags["C_CONTIGUOUS"] and w.size == 2 * 16 + 16 + 2
    assert (plan.batch, plan.n_supports, plan.q_off, plan.s_off) == (2, 1, 0, 32)
    assert w[[0, 1]].tolist() == [1, 2] and w[6:14].tolist() == [0, 9, 48, 60, 59, -1, 2, 48] and w[48:50].tolist() == [1, 0]
    assert w[2:6].view(np.float64).tolist() == [48.0 / 37.0, 1.0 / (48.0 / 37.0)]
    assert w[16:18].tolist() == [4, 0] and w[16 + 13] == 50  # no boxes: an empty order behind the first one
    s = w[32:48]
    # 64x48 at 48: scale 1, the box as it is; 58 rows > 38 columns -> rh = 32, rw = int(38 * (32 / 58)) = 20
    assert s[0] == 2 and s[8:16].tolist() == [2, 2, 39, 59, 20, 32, 64, 48] and w[14:16].tolist() == [48, 69]
    assert s[2:8].view(np.float64).tolist() == [1.0, 39 / 20, 59 / 32]


def test_plan_support_boxes(pool):
    def sup(row, box, target=48, size=32):
        return PL.plan_episode(pool, (), [(row, box)], target_size=target, support_size=size).supports[0]
    # scale 48/37 = 1.297...: (3, 4, 30, 20) -> int16 (3, 5, 38, 25); box_w 35 > box_h 20 -> rw = 32, rh = int(20 * (32 / 35)) = 18
    s = sup(1, (3, 4, 30, 20))
    assert (s["x_min"], s["y_min"], s["x_max"], s["y_max"], s["rw"], s["rh"]) == (3, 5, 38, 25, 32, 18)
    assert (s["cw"], s["ch"], s["oh"], s["ow"]) == (36, 21, 48, 69)
    # box_h > box_w: (2, 2, 40, 60) at scale 1 -> 58 rows, 38 columns
    s = sup(2, (2, 2, 40, 60))
    assert (s["rw"], s["rh"], s["cw"], s["ch"]) == (20, 32, 39, 59)
    # touching the right / bottom border: 53 * 1.297 = 68.76 -> 68, 54.5 * 1.297 = 70.7 -> 70 > ow - 1 = 68: x_max is limited
    # to 68, the crop is ONE pixel wide, and rw still comes from the unlimited box (box_w = 2, box_h = 40 -> int(2 * 0.8) = 1)
    s = sup(1, (53, 5, 54.5, 36))
    assert (s["x_min"], s["x_max"], s["y_min"], s["y_max"]) == (68, 68, 6, 46) and (s["cw"], s["ch"], s["rw"], s["rh"]) == (1, 41, 1, 32)
    s = sup(0, (0, 0, 7, 5))  # 5x7 at 48: scale 9.6, oh 48, ow round(67.2) = 67; (0, 0, 67, 48) limited to (66, 47)
    assert (s["x_max"], s["y_max"], s["cw"], s["ch"], s["rw"], s["rh"]) == (66, 47, 67, 48, 32, 22)


def test_plan_refusals(pool):
    hw = (48, 64)
    ok = dict(row=1, ratio=1.25, pos_cls=1, need_crop=True, crop_start=9)
    PL.plan_episode(pool, [ok], holder_hw=hw, target_size=48)
    with pytest.raises(ValueError, match="leaves the prepared image"):  # 10 + 60 > 69
        PL.plan_episode(pool, [dict(ok, crop_start=10)], holder_hw=hw, target_size=48)
    with pytest.raises(ValueError, match="leaves the prepared image"):
        PL.plan_episode(pool, [dict(ok, crop_start=-1)], holder_hw=hw, target_size=48)
    with pytest.raises(ValueError, match="larger than the holder"):  # 48 x 69 into 48 x 64
        PL.plan_episode(pool, [dict(row=1, ratio=1.5, pos_cls=1)], holder_hw=hw, target_size=48)
    with pytest.raises(ValueError, match="box order"):
        PL.plan_episode(pool, [dict(row=1, ratio=1.0, pos_cls=1, order=[0, 2])], holder_hw=hw, target_size=48)
    with pytest.raises(ValueError, match="holder_hw"):
        PL.plan_episode(pool, [dict(row=1, ratio=1.0, pos_cls=1)], target_size=48)
    for row in (-1, 5):
        with pytest.raises(IndexError):
            PL.plan_episode(pool, [dict(row=row, ratio=1.0, pos_cls=1)], holder_hw=hw, target_size=48)
        with pytest.raises(IndexError):
            PL.plan_episode(pool, (), [(row, (0, 0, 3, 3))], target_size=48)
    with pytest.raises(ValueError, match="resizes to 0 x 32"):  # a box of one column: box_w = 0
        PL.plan_episode(pool, (), [(1, (15, 7, 15, 30))], target_size=48, support_size=32)
    with pytest.raises(ValueError, match="resizes to"):  # 30 columns, 1 row of height 1 -> rh = int(1 * 32 / 38) = 0
        PL.plan_episode(pool, (), [(1, (3, 4, 33, 5))], target_size=48, support_size=32)
    with pytest.raises(ValueError, match="outside its image"):  # starts right of the last prepared column
        PL.plan_episode(pool, (), [(1, (54, 4, 60, 20))], target_size=48)
    with pytest.raises(ValueError, match="outside its image"):
        PL.plan_episode(pool, (), [(1, (-3, 4, 30, 20))], target_size=48)
    with pytest.raises(ValueError, match="outside its image"):  # x_max < x_min
        PL.plan_episode(pool, (), [(1, (30, 4, 3, 40))], target_size=48)


def test_plan_refuses_device_tensors(pool):
    class _Dev:  # stands for a device tensor where there is no device: the check reads `is_cuda`
        is_cuda = True
    with pytest.raises(ValueError, match="device tensor"):
        PL.plan_episode(pool, [dict(row=1, ratio=1.0, pos_cls=1, order=_Dev())], holder_hw=(48, 64), target_size=48)
    with pytest.raises(ValueError, match="device tensor"):
        PL.plan_episode(pool, [dict(row=_Dev(), ratio=1.0, pos_cls=1)], holder_hw=(48, 64), target_size=48)
    with pytest.raises(ValueError, match="device tensor"):
        PL.plan_episode(pool, (), [(1, _Dev())], target_size=48)
    # host tensors are fine
    p = PL.plan_episode(pool, [dict(row=1, ratio=1.0, pos_cls=1, order=torch.tensor([1, 0]))], holder_hw=(48, 64), target_size=48)
    assert p.queries[0]["order"].tolist() == [1, 0]


# ---- test 2: episode_boxes_numpy ---------------------------------------------------------------------------------------
def box_cases():
    """name -> (boxes, order, im_scale, x_s, y_s, clamp_x, clamp_y, pos_cls, max_num_box), (fs rows, all rows) expected
    before zero padding. Shared with the device test."""
    c = {}
    c["no boxes"] = ((np.zeros((0, 5)), [], 1.5, 0, 0, -1, -1, 1, 4), ([], []))
    # five boxes, three of class 2 and two of class 1, into three rows: in order, cut at max_num_box
    many = [[0, 0, 2, 2, 2], [1, 1, 3, 3, 1], [2, 2, 4, 4, 2], [3, 3, 5, 5, 2], [4, 4, 6, 6, 1]]
    c["more than max_num_box"] = ((many, [0, 1, 2, 3, 4], 2.0, 0, 0, -1, -1, 2, 2),
                                  ([[0, 0, 4, 4, 1], [4, 4, 8, 8, 1]], [[0, 0, 4, 4, 2], [2, 2, 6, 6, 1]]))
    c["another class"] = ((many, [4, 3, 2, 1, 0], 1.0, 0, 0, -1, -1, 3, 4),
                          ([], [[4, 4, 6, 6, 1], [3, 3, 5, 5, 2], [2, 2, 4, 4, 2], [1, 1, 3, 3, 1]]))
    # x crop from 20 with trim 30: [0, 29]. Box 0 lies left of the window (both x clamp to 0: dropped), box 1 right of it
    # (both 29: dropped), box 2 straddles the left edge, box 3 is inside; y is not clamped
    crop = [[2, 5, 18, 40, 1], [52, 5, 60, 40, 1], [10, 5, 30, 40, 1], [25, 6, 45, 50, 1]]
    c["degenerate after the crop clamp"] = ((crop, [0, 1, 2, 3], 1.0, 20, 0, 29, -1, 1, 4),
                                            ([[0, 5, 10, 40, 1], [5, 6, 25, 50, 1]], [[0, 5, 10, 40, 1], [5, 6, 25, 50, 1]]))
    # ratio == 1 with trim 48: 48 itself survives the clamp (a box from 48 to 60 collapses, one from 40 to 60 ends at 48)
    sq = [[40, 10, 60, 70, 1], [48, 10, 60, 20, 1], [5, 48, 9, 50, 1]]
    c["ratio 1 clamps to trim"] = ((sq, [0, 1, 2], 1.0, 0, 0, 48, 48, 1, 4), ([[40, 10, 48, 48, 1]], [[40, 10, 48, 48, 1]]))
    # compaction keeps the plan's order: the shuffled order [3, 0, 2, 1] minus the dropped box 1 (x1 == x2)
    mixed = [[1, 1, 5, 5, 1], [7, 2, 7, 9, 1], [2, 2, 6, 6, 2], [3, 3, 8, 8, 1]]
    c["order kept"] = ((mixed, [3, 0, 2, 1], 1.0, 0, 0, -1, -1, 1, 4),
                       ([[3, 3, 8, 8, 1], [1, 1, 5, 5, 1]], [[3, 3, 8, 8, 1], [1, 1, 5, 5, 1], [2, 2, 6, 6, 2]]))
    # y crop: the other axis, shifted by 7 and clamped to [0, 19]
    c["y crop"] = (([[3, 10, 9, 40, 1]], [0], 1.0, 0, 7, -1, 19, 1, 2), ([[3, 3, 9, 19, 1]], [[3, 3, 9, 19, 1]]))
    return c


@pytest.mark.parametrize("name", sorted(box_cases()))
def test_episode_boxes_numpy_hand_cases(name):
    args, (fs_rows, all_rows) = box_cases()[name]
    fs, n_fs, al, n_al = PL.episode_boxes_numpy(np.asarray(args[0], dtype=np.float32), *args[1:])
    mx = args[-1]
    assert fs.shape == al.shape == (mx, 5) and fs.dtype == al.dtype == np.float32
    assert n_fs == len(fs_rows) and n_al == len(all_rows)
    for got, n, rows in ((fs, n_fs, fs_rows), (al, n_al, all_rows)):
        assert np.array_equal(got[:n], np.asarray(rows, dtype=np.float32).reshape(n, 5))
        assert not got[n:].any()


def test_episode_boxes_numpy_scales_in_double():
    """minibatch.py:53 multiplies in double and the float32 array rounds once. At scale 1.6 (a 375 x 500 image at 600) the
    coordinate 9 gives float32(14.4) = 14.399999618530273 that way and 14.40000057220459 as a float32 product (float32(1.6)
    is above 1.6)."""
    scale = 600.0 / 375.0
    one_rounding, float_product = np.float32(np.float64(9.0) * scale), np.float32(9.0) * np.float32(scale)
    assert float(one_rounding) == 14.399999618530273 and float(float_product) == 14.40000057220459
    fs, n, _, _ = PL.episode_boxes_numpy(np.array([[9, 9, 18, 13, 1]], dtype=np.float32), [0], scale, 0, 0, -1, -1, 1, 1)
    assert n == 1
    assert [float(v) for v in fs[0]] == [14.399999618530273, 14.399999618530273, 28.799999237060547, 20.799999237060547, 1.0]


def test_plan_boxes_numpy_uses_the_plan(pool):
    plan = PL.plan_episode(pool, [dict(row=1, ratio=1.25, pos_cls=2, need_crop=True, crop_start=9, order=[1, 0]),
                                  dict(row=4, ratio=1.25, pos_cls=1)], holder_hw=(48, 64), target_size=48)
    fs, n_fs, al, n_al = plan.boxes_numpy(pool, 3)
    assert fs.shape == al.shape == (2, 3, 5) and n_fs.tolist() == [1, 0] and n_al.tolist() == [2, 0]
    s = 48.0 / 37.0  # box 1 = (10, 5, 50, 36, 2): x shifted by 9 (64.86 - 9 stays below the clamp at 59), y untouched
    want = [np.float32(10 * s) - np.float32(9), np.float32(5 * s), np.float32(50 * s) - np.float32(9), np.float32(36 * s),
            np.float32(1)]
    assert fs[0, 0].tolist() == [float(v) for v in want]
    assert al[0, 0, 4] == 2 and al[0, 1, 4] == 1 and not fs[1].any() and not al[1].any()
