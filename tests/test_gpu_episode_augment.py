"""Training-time augmentation in the episode assembler (csrc/episode.hip's *_aug launches through pipeline.plan_episode /
EpisodeAssembler) on the small pool of test_gpu_episode_assembler.py.

What is compared with what:
  * identity records through the augmented launches      == the plain launches of the same plan, bit for bit
  * maps with integer results (permutation, 255 - v, ...) == the plain launches on a pool of frames distorted on the host,
                                                            bit for bit: the reference is code this feature does not touch
  * general matrices                                      == numpy's float32 tap expression at identity scale, bit for bit;
                                                            oracle/pipeline_ref.py on the distorted float image elsewhere,
                                                            within the 2e-4 test_gpu_pipeline.py gives that comparison (the
                                                            clamp keeps tap values in the range of undistorted pixels)
  * per-query scales, crop windows                        == plain plans / the per-image path, bit for bit
  * the visibility rule                                   == pipeline.episode_boxes_numpy, bit for bit, with every
                                                            seen / full ratio a relative VIS_GAP away from the threshold"""
import numpy as np
import pytest
import torch

from test_gpu_episode_assembler import MEANS, QUERY_CASES, SMALL, SUPPORTS, make_pool, per_image, same

pytestmark = pytest.mark.gpu

# The kernel and numpy evaluate seen >= f * full in float32 from float32 coordinates: three roundings of 2^-24 each on
# either side. A case whose seen / full lies within 1e-3 (relative) of f is not a test of the rule but of those roundings,
# so every case below is checked on the host to keep this gap.
VIS_GAP = 1e-3


def _identity_queries(queries):
    from dana_amd import pipeline as PL
    return [dict(q, color=PL.color_matrix(), min_visible=0.0) for q in queries]


def _assemble(dev, pool, plan, ws, support_size=32, nb=4):
    from dana_amd import pipeline as PL
    H, W = plan.holder_hw
    hold = PL.EpisodeHolders(plan.batch, 1, ws, H, W, dev, support_size=support_size, max_num_box=nb)
    for t in hold.tensors():
        t.fill_(7)
    asm = PL.EpisodeAssembler(pool, hold, pixel_means=MEANS)
    out = asm.assemble(plan)
    torch.cuda.synchronize()
    return list(out) + [asm.all_cls_num_boxes]


def _case(name):
    """-> (target, holder, queries, supports): a QUERY_CASES entry with all six SUPPORTS spread over its batch items"""
    target, hw, queries = QUERY_CASES[name]
    return target, hw, queries, SUPPORTS, len(SUPPORTS) // len(queries)


# ---- identity: the augmented launches with nothing to do -----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(QUERY_CASES))
def test_identity_records_give_the_plain_bits(dev, name):
    from dana_amd import pipeline as PL
    target, hw, queries, sups, ws = _case(name)
    pool, _ = make_pool(dev, SMALL)
    plain = PL.plan_episode(pool, queries, sups, holder_hw=hw, target_size=target, support_size=32)
    aug = PL.plan_episode(pool, _identity_queries(queries), [s + (PL.color_matrix(),) for s in sups], holder_hw=hw,
                          target_size=target, support_size=32)
    assert aug.augmented and not plain.augmented and np.array_equal(aug.words[:plain.words.size], plain.words)
    flags = aug.words[aug.a_off + PL.A_FLAGS::PL.EP_AWORDS]
    assert flags.tolist() == [PL.A_HAS_COLOR] * (len(queries) + len(sups))
    got, want = _assemble(dev, pool, aug, ws), _assemble(dev, pool, plain, ws)
    same(got, want)  # im_data, im_info, gt_boxes, num_boxes, support_ims, all_cls_gt_boxes and its counts
    assert float(got[0].abs().max()) > 1 and int(got[3].sum()) > 0 and int(got[6].sum()) > 0
    assert all(float(got[4][b, n].abs().max()) > 1 for b in range(len(queries)) for n in range(ws))
    assert not (got[0] == 7).all() and not (got[4] == 7).any()


@pytest.mark.parametrize("target", [48, 32])
def test_identity_support_crops_give_the_plain_bits(dev, target):
    from dana_amd import pipeline as PL
    pool, _ = make_pool(dev, SMALL)
    asm = PL.EpisodeAssembler(pool, pixel_means=MEANS, support_size=32)
    plain = PL.plan_episode(pool, (), SUPPORTS, target_size=target, support_size=32)
    aug = PL.plan_episode(pool, (), [s + (PL.color_matrix(),) for s in SUPPORTS], target_size=target, support_size=32)
    assert aug.augmented and aug.batch == 0 and plain.supports[0]["cw"] == 1
    got, want = asm.support_crops(aug), asm.support_crops(plain)
    assert torch.equal(got, want) and all(float(got[n].abs().max()) > 1 for n in range(len(SUPPORTS)))


# ---- maps with integer results against the plain launches on distorted frames --------------------------------------------
def _exact_maps():
    eye = np.eye(3, 4, dtype=np.float32)
    perm = np.zeros((3, 4), dtype=np.float32)
    perm[0, 2] = perm[1, 0] = perm[2, 1] = 1  # R' = b, G' = r, B' = g
    neg = -eye
    neg[:, 3] = 255
    up, down = eye.copy(), eye.copy()
    up[:, 3], down[:, 3] = 40, -300
    return {"permutation": (perm, lambda im: im[..., [2, 0, 1]]),
            "255 - v": (neg, lambda im: 255 - im),
            "v + 40 saturates": (up, lambda im: np.minimum(im.astype(np.int32) + 40, 255).astype(np.uint8)),
            "v - 300 is 0": (down, lambda im: np.zeros_like(im))}


def _distorted_pool(dev, src, fn):
    """the pool of `make_pool(dev, SMALL)` with every frame distorted on the host; flipped twins share the distorted frame"""
    from dana_amd import pipeline as PL
    pool = PL.ImagePool(dev)
    for spec, (im, _) in zip(SMALL, src):
        if spec[0] == "flip":
            pool.add_flipped(spec[1], spec[2])
        else:
            pool.add(np.ascontiguousarray(fn(im)), spec[2])
    return pool.freeze()


@pytest.mark.parametrize("case", ["up_crop_flip", "down_pad_both"])
@pytest.mark.parametrize("name", sorted(_exact_maps()))
def test_exact_maps_equal_the_plain_path_on_distorted_frames(dev, name, case):
    from dana_amd import pipeline as PL
    m, fn = _exact_maps()[name]
    target, hw, queries, sups, ws = _case(case)
    pool, src = make_pool(dev, SMALL)
    pool2 = _distorted_pool(dev, src, fn)
    assert np.array_equal(PL.apply_color_numpy(src[1][0], m), fn(src[1][0]).astype(np.float32))  # the map IS that distortion
    aug = PL.plan_episode(pool, [dict(q, color=m) for q in queries], [s + (m,) for s in sups], holder_hw=hw,
                          target_size=target, support_size=32)
    plain = PL.plan_episode(pool2, queries, sups, holder_hw=hw, target_size=target, support_size=32)
    assert aug.augmented and not plain.augmented
    got, want = _assemble(dev, pool, aug, ws), _assemble(dev, pool2, plain, ws)
    same(got, want)
    undistorted = _assemble(dev, pool, PL.plan_episode(pool, queries, sups, holder_hw=hw, target_size=target, support_size=32), ws)
    assert not torch.equal(got[0], undistorted[0]) and not torch.equal(got[4], undistorted[4])
    asm, asm2 = PL.EpisodeAssembler(pool, pixel_means=MEANS, support_size=32), PL.EpisodeAssembler(pool2, pixel_means=MEANS, support_size=32)
    crops = asm.support_crops(PL.plan_episode(pool, (), [s + (m,) for s in sups], target_size=target, support_size=32))
    assert torch.equal(crops, asm2.support_crops(PL.plan_episode(pool2, (), sups, target_size=target, support_size=32)))


# ---- general matrices ------------------------------------------------------------------------------------------------------
def _general_maps():
    from dana_amd import pipeline as PL
    drawn = PL.draw_color_matrix(np.random.default_rng(2024), p=1.0)
    assert not np.array_equal(drawn, np.eye(3, 4, dtype=np.float32))
    return {"fixed": PL.color_matrix(-12, 1.3, 0.6, 17), "drawn": drawn}


def _distorted_bgr(im, flipped, m):
    """the image the resamples see: distorted (float32, clamped, never rounded to uint8), BGR, mirrored, mean-subtracted"""
    from dana_amd import pipeline as PL
    d = PL.apply_color_numpy(im, m)[:, :, ::-1]
    if flipped:
        d = d[:, ::-1, :]
    return np.ascontiguousarray(d - MEANS.reshape(1, 1, 3))


@pytest.mark.parametrize("which", ["fixed", "drawn"])
def test_general_matrix_at_identity_scale_is_the_tap_expression(dev, which):
    """the 64x48 row at target 48: im_scale 1, every tap weight 1 or 0, so the output IS the distorted tap minus the mean"""
    from dana_amd import pipeline as PL
    m = _general_maps()[which]
    pool, src = make_pool(dev, SMALL)
    plan = PL.plan_episode(pool, [dict(row=2, ratio=0.75, pos_cls=1, color=m)], holder_hw=(64, 48), target_size=48)
    assert plan.queries[0]["im_scale"] == 1.0 and (plan.queries[0]["copy_h"], plan.queries[0]["copy_w"]) == (64, 48)
    got = _assemble(dev, pool, plan, 0)[0][0].cpu().numpy()
    want = np.transpose(_distorted_bgr(src[2][0], False, m), (2, 0, 1))
    assert got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()
    if which == "fixed":  # both clamps and the open range are exercised
        d = PL.apply_color_numpy(src[2][0], m)
        assert (d == 0).any() and (d == 255).any() and ((d > 0) & (d < 255)).any()


@pytest.mark.parametrize("case", ["up_crop_flip", "down_pad_both"])
@pytest.mark.parametrize("which", ["fixed", "drawn"])
def test_general_matrix_against_the_restatement(dev, which, case):
    from dana_amd import pipeline as PL
    from oracle import pipeline_ref as P
    m = _general_maps()[which]
    target, hw, queries, sups, ws = _case(case)
    pool, src = make_pool(dev, SMALL)
    plan = PL.plan_episode(pool, [dict(q, color=m) for q in queries], [s + (m,) for s in sups], holder_hw=hw,
                           target_size=target, support_size=32)
    got = _assemble(dev, pool, plan, ws)
    prepared = {}

    def prep(row, im_scale):
        if row not in prepared:
            prepared[row] = P.cv_resize_linear(_distorted_bgr(src[row][0], src[row][1], m), fx=im_scale, fy=im_scale)
        return prepared[row]

    for b, q in enumerate(plan.queries):
        im = prep(q["row"], q["im_scale"])
        assert im.shape[:2] == (q["oh"], q["ow"])
        want = P.crop_pad_chw(im, q["y_s"], q["x_s"], q["copy_h"], q["copy_w"], hw[0], hw[1])
        err = float(np.abs(got[0][b].cpu().numpy() - want).max())
        print(case, which, "query", b, "max |diff|", err)
        assert err <= 2e-4
    for n, ((row, box), s) in enumerate(zip(sups, plan.supports)):
        sb = (np.array(box, dtype=np.float32) * s["im_scale"]).astype(np.int16)  # fs_loader.py:120
        want = P.support_crop(prep(row, s["im_scale"]), sb, 32)
        err = float(np.abs(got[4][n // ws, n % ws].cpu().numpy() - want).max())
        print(case, which, "support", n, "max |diff|", err)
        assert err <= 2e-4
    plain = _assemble(dev, pool, PL.plan_episode(pool, queries, sups, holder_hw=hw, target_size=target, support_size=32), ws)
    assert float((got[0] - plain[0]).abs().max()) > 1 and float((got[4] - plain[4]).abs().max()) > 1
    same(got[2:4] + got[5:], plain[2:4] + plain[5:])  # colour leaves the boxes alone


# ---- per-query scales --------------------------------------------------------------------------------------------------------
MULTI_SCALE = [dict(row=1, ratio=1.0, pos_cls=1, target_size=48),
               dict(row=2, ratio=0.75, pos_cls=1, target_size=32, order=[2, 0, 1]),
               dict(row=3, ratio=1.25, pos_cls=2, need_crop=True, crop_start=2, target_size=40)]


@pytest.mark.parametrize("through", ["plain launches", "augmented launches"])
def test_per_query_scales_equal_one_plan_per_scale(dev, through):
    from dana_amd import pipeline as PL
    pool, _ = make_pool(dev, SMALL)
    queries = MULTI_SCALE if through == "plain launches" else _identity_queries(MULTI_SCALE)
    multi = PL.plan_episode(pool, queries, holder_hw=(48, 64), target_size=600)  # (the global scale is overridden everywhere)
    assert multi.augmented == (through == "augmented launches")
    assert [q["im_scale"] for q in multi.queries] == [48 / 37.0, 32 / 48.0, 40 / 37.0]
    got = _assemble(dev, pool, multi, 0)
    for b, q in enumerate(MULTI_SCALE):
        one = {k: v for k, v in q.items() if k != "target_size"}
        want = _assemble(dev, pool, PL.plan_episode(pool, [one], holder_hw=(48, 64), target_size=q["target_size"]), 0)
        same([t[b:b + 1] for t in got[:4] + got[5:]], want[:4] + want[5:])
        assert float(want[0].abs().max()) > 1 and int(want[6].sum()) > 0


# ---- crop windows: pixels and boxes ------------------------------------------------------------------------------------------
def _visible_fractions(boxes, order, im_scale, x_s, y_s, clamp_x, clamp_y):
    """seen / full per box in float64, for the margin check (nan where the unclamped box has no area)"""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 5)[np.asarray(order, dtype=np.int64)]
    u = b[:, :4] * im_scale - np.array([x_s, y_s, x_s, y_s], dtype=np.float64)
    v = u.copy()
    if clamp_x >= 0:
        v[:, 0::2] = np.clip(v[:, 0::2], 0, clamp_x)
    if clamp_y >= 0:
        v[:, 1::2] = np.clip(v[:, 1::2], 0, clamp_y)
    full = (u[:, 2] - u[:, 0]) * (u[:, 3] - u[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(full > 0, (v[:, 2] - v[:, 0]) * (v[:, 3] - v[:, 1]) / full, np.nan)


def _keeps_the_gap(fractions, f):
    r = fractions[~np.isnan(fractions)]
    return bool((np.abs(r - f) >= VIS_GAP * f).all())


def test_crop_window_pixels_and_boxes_equal_the_per_image_path(dev):
    """free windows of the prepared images (one reaching the last prepared row and column, one cut by the holder), with and
    without a visibility threshold: im_data equals put_query with the same y_s, x_s, copy_h, copy_w; the boxes equal
    episode_boxes_numpy"""
    from dana_amd import pipeline as PL
    pool, src = make_pool(dev, SMALL)
    queries = [dict(row=1, pos_cls=1, crop=(5, 30, 40, 30), min_visible=0.3),   # 48 x 69 prepared: an inner window
               dict(row=3, pos_cls=1, crop=(8, 9, 40, 60)),                     # the flipped twin, to its last row and column
               dict(row=0, pos_cls=2, crop=(0, 0, 48, 67), order=[1, 0]),       # the whole 48 x 67: cut to the holder's 64
               dict(row=2, pos_cls=1, crop=(30, 10, 30, 38), min_visible=0.5, color=PL.color_matrix())]
    plan = PL.plan_episode(pool, queries, holder_hw=(48, 64), target_size=48)
    assert plan.augmented and [(q["copy_h"], q["copy_w"]) for q in plan.queries] == [(40, 30), (40, 60), (48, 64), (30, 38)]
    assert (plan.queries[2]["clamp_x"], plan.queries[2]["clamp_y"]) == (66, 47)
    for q in plan.queries:
        if q["min_visible"]:
            fr = _visible_fractions(pool.row_boxes(q["row"]), q["order"], q["im_scale"], q["x_s"], q["y_s"], q["clamp_x"], q["clamp_y"])
            assert _keeps_the_gap(fr, q["min_visible"]), fr
    got = _assemble(dev, pool, plan, 0)
    ref, ref_all = per_image(dev, pool, src, plan, [], 48, 0, 32, 4)
    same(got[:4] + got[5:6], list(ref.tensors()[:4]) + [ref_all])
    fs, n_fs, al, n_al = plan.boxes_numpy(pool, 4)
    assert got[3].tolist() == n_fs.tolist() and got[6].tolist() == n_al.tolist()
    without = PL.plan_episode(pool, [{k: v for k, v in q.items() if k != "min_visible"} for q in queries], holder_hw=(48, 64),
                              target_size=48).boxes_numpy(pool, 4)
    assert n_al.tolist() == [2, 2, 2, 1] and without[3].tolist() == [3, 2, 2, 2]  # the rule dropped a box of items 0 and 3
    assert float(got[0].abs().max()) > 1


def _run_boxes_aug(dev, boxes, order, im_scale, x_s, y_s, clamp_x, clamp_y, pos_cls, mx, f):
    """dana_episode_boxes_aug for one image whose records carry exactly these numbers"""
    from dana_amd import pipeline as PL
    from dana_amd._lib import lib
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 5)
    pool = PL.ImagePool(dev)
    pool.add(np.zeros((4, 4, 3), dtype=np.uint8), boxes)
    pool.freeze()
    plan = PL.plan_episode(pool, [dict(row=0, ratio=1.0, pos_cls=pos_cls, order=order, min_visible=f)], holder_hw=(4, 4), target_size=4)
    w = plan.words
    assert plan.augmented and w[plan.a_off + PL.A_FLAGS] == (PL.A_HAS_VISIBLE if f > 0 else 0)
    w[PL.Q_SCALE:PL.Q_SCALE + 2].view(np.float64)[0] = im_scale
    w[PL.Q_YS], w[PL.Q_XS], w[PL.Q_CLAMP_X], w[PL.Q_CLAMP_Y] = y_s, x_s, clamp_x, clamp_y
    d_plan = torch.from_numpy(w).to(dev)
    fs = torch.full((1, mx, 5), 7.0, device=dev)
    al = torch.full((1, mx, 5), 7.0, device=dev)
    n_fs = torch.full((1,), -1, dtype=torch.long, device=dev)
    n_al = torch.full((1,), -1, dtype=torch.long, device=dev)
    lib().call("dana_episode_boxes_aug", pool.d_boxes.data_ptr(), len(pool.boxes), pool.d_meta.data_ptr(), 1, d_plan.data_ptr(),
               int(w.size), 0, plan.a_off, 1, mx, fs.data_ptr(), n_fs.data_ptr(), al.data_ptr(), n_al.data_ptr(),
               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return fs[0].cpu().numpy(), int(n_fs), al[0].cpu().numpy(), int(n_al)


def _two_pass_boxes():
    """100 boxes in shuffled order against the x window [50, 149] (clamp 99), y free: 40 wide, starting at 60 (inside: 1),
    30 (half: 0.5), 20 (a quarter: 0.25), 0 (left of the window: degenerate) or 120 (29 of 40 = 0.725); two classes"""
    rng = np.random.RandomState(12)
    kinds = np.array([60, 30, 20, 0, 120], dtype=np.float32)[rng.randint(0, 5, size=100)]
    b = np.zeros((100, 5), dtype=np.float32)
    b[:, 0], b[:, 2] = kinds, kinds + 40
    b[:, 1] = rng.randint(0, 50, size=100)
    b[:, 3] = b[:, 1] + rng.randint(1, 30, size=100)
    b[:, 4] = rng.randint(1, 3, size=100)
    return b, rng.permutation(100)


def _vis_cases():
    """name -> (boxes, order, im_scale, x_s, y_s, clamp_x, clamp_y, pos_cls, max_num_box, f)"""
    # window x [20, 49], y [10, 39]: inside; outside (right of it); cut in half by the left edge (x 5..35 -> -15..15 -> 0..15)
    three = [[25, 15, 45, 35, 1], [60, 15, 80, 35, 1], [5, 12, 35, 30, 1]]
    c = {"window, half-cut kept at 0.4": (three, [0, 1, 2], 1.0, 20, 10, 29, 29, 1, 4, 0.4),
         "window, half-cut dropped at 0.6": (three, [0, 1, 2], 1.0, 20, 10, 29, 29, 1, 4, 0.6),
         "window, no rule": (three, [2, 1, 0], 1.0, 20, 10, 29, 29, 1, 4, 0.0),
         # scaled by 1.6 in double first: (10, 10, 30, 30) -> 16..48, - 24 -> -8..24 of 32: 0.75 in x, whole in y
         "scaled": ([[10, 10, 30, 30, 1], [0, 10, 20, 30, 1]], [0, 1], 600.0 / 375.0, 24, 0, 99, -1, 1, 4, 0.5),
         # the cut at max_num_box = 2 falls after the dropped box 1: rows 0 and 2 stay, 3 is cut
         "cut after a dropped box": ([[25, 15, 45, 35, 1], [5, 12, 27, 30, 1], [22, 11, 40, 30, 1], [30, 20, 44, 38, 1]],
                                     [0, 1, 2, 3], 1.0, 20, 10, 29, 29, 1, 2, 0.5)}
    b, order = _two_pass_boxes()
    c["100 boxes, two passes"] = (b, order, 1.0, 50, 0, 99, -1, 2, 100, 0.4)
    c["100 boxes, cut at 20"] = (b, order, 1.0, 50, 0, 99, -1, 1, 20, 0.6)
    return c


@pytest.mark.parametrize("name", sorted(_vis_cases()))
def test_visibility_rule_equals_the_numpy_restatement(dev, name):
    from dana_amd import pipeline as PL
    args = _vis_cases()[name]
    boxes, f = np.asarray(args[0], dtype=np.float32), args[-1]
    fr = _visible_fractions(boxes, *args[1:7])
    if f > 0:
        assert _keeps_the_gap(fr, f), fr
    want = PL.episode_boxes_numpy(boxes, *args[1:9], min_visible=f)
    ruleless = PL.episode_boxes_numpy(boxes, *args[1:9])
    got = _run_boxes_aug(dev, boxes, *args[1:])
    print(name, "num_boxes", got[1], got[3], "expected", want[1], want[3], "without the rule", ruleless[1], ruleless[3])
    assert isinstance(got[1], int) and got[1] == want[1] and got[3] == want[3]
    assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()
    if name == "window, half-cut kept at 0.4":
        assert want[3] == 2 and want[2][1].tolist() == [0, 2, 15, 20, 1]
    if name == "window, half-cut dropped at 0.6":
        assert want[3] == 1 and ruleless[3] == 2
    if name == "cut after a dropped box":
        assert want[3] == 2 and want[2][:2, :4].tolist() == [[5, 5, 25, 25], [2, 1, 20, 20]] and ruleless[2][1, :4].tolist() == [0, 2, 7, 20]
    if name == "100 boxes, two passes":
        by_rule = np.array([not np.isnan(r) and 0 < r < f for r in fr])
        assert by_rule[:64].any() and by_rule[64:].any()  # drops in both 64-lane passes
        assert want[3] < ruleless[3] and want[1] < ruleless[1]


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_augmented_batch_feeds_a_training_forward(dev):
    """bs 2, way 1, shot 1 at 128 x 160: colour on every record, a crop window, a visibility threshold and two scales, then one
    train-mode forward; and the holders stay where they are between an augmented and a plain assemble"""
    import dana_amd
    from dana_amd import pipeline as PL, synthetic as S
    specs = [(100, 130, [[10, 12, 90, 80, 1], [60, 30, 128, 95, 2]]), (120, 150, [[20, 20, 100, 100, 1], [0, 50, 40, 110, 1]])]
    pool, _ = make_pool(dev, specs, seed=6)
    rng = np.random.default_rng(9)
    queries = [dict(row=0, pos_cls=1, target_size=128, crop=(0, 3, 128, 160), min_visible=0.3, color=PL.draw_color_matrix(rng, p=1.0)),
               dict(row=1, ratio=1.25, pos_cls=1, target_size=128, color=PL.draw_color_matrix(rng, p=1.0))]
    sups = [(1, (20, 20, 100, 100), PL.draw_color_matrix(rng, p=1.0)), (0, (10, 12, 90, 80), PL.draw_color_matrix(rng, p=1.0))]
    assert PL.scales_holder_hw(pool, [0, 1], (128,)) == (128, 166)
    plan = PL.plan_episode(pool, queries, sups, holder_hw=(128, 160))
    plain = PL.plan_episode(pool, [dict(row=0, pos_cls=1, target_size=128, crop=(0, 3, 128, 160)),
                                   dict(row=1, ratio=1.25, pos_cls=1, target_size=128)], [s[:2] for s in sups], holder_hw=(128, 160))
    assert plan.augmented and not plain.augmented
    hold = PL.EpisodeHolders(2, 1, 1, 128, 160, dev)
    asm = PL.EpisodeAssembler(pool, hold, pixel_means=MEANS)
    where = [t.data_ptr() for t in hold.tensors()] + [asm.all_cls_gt_boxes.data_ptr()]
    out_plain = [t.clone() for t in asm.assemble(plain)]
    assert [t.data_ptr() for t in asm.assemble(plan)] == where
    out = asm.assemble(plan)
    assert [t.data_ptr() for t in out] == where == [t.data_ptr() for t in hold.tensors()] + [asm.all_cls_gt_boxes.data_ptr()]
    assert not torch.equal(out[0], out_plain[0]) and not torch.equal(out[4], out_plain[4]) and int(out[3].min()) >= 1
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=1, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=4, profile="test"))
    m.to(dev).train()
    np.random.seed(11)
    with torch.no_grad():
        res = m(*out[:5])
    torch.cuda.synchronize()
    assert len(res) == 8 and all(torch.isfinite(torch.as_tensor(t).float()).all() for t in res)
