"""A batch of episodes assembled from a resident image pool (csrc/episode.hip through pipeline.EpisodeAssembler) against the
per-image path of the same build (prep_im_for_blob -> crop_pad_chw / support_crop -> EpisodeHolders.put_*), which
test_gpu_pipeline.py pins to oracle/pipeline_ref.py. Every comparison is bit for bit: the new kernels evaluate the same
expressions in the same order, so any difference is a bug in them."""
import numpy as np
import pytest
import torch

from test_episode_plan_host import box_cases

pytestmark = pytest.mark.gpu

MEANS = np.array([102.9801, 115.9465, 122.7717], dtype=np.float32)
# (h, w, boxes) per row; ("flip", twin, boxes) for a flipped twin
SMALL = [(5, 7, [[1, 1, 4, 3, 2], [0, 0, 6, 4, 1]]),
         (37, 53, [[3, 4, 30, 20, 1], [10, 5, 50, 36, 2], [0, 0, 52, 36, 1]]),
         (64, 48, [[2, 2, 40, 60, 1], [30, 40, 47, 63, 1], [5, 5, 5, 30, 1]]),
         ("flip", 1, [[22, 4, 49, 20, 1], [2, 5, 42, 36, 2]])]


def make_pool(dev, specs, seed=0):
    """-> (frozen ImagePool on dev, [(host image, flipped)] per row); odd rows go in as device tensors"""
    from dana_amd import pipeline as PL
    rng = np.random.RandomState(seed)
    pool, src = PL.ImagePool(dev), []
    for spec in specs:
        if spec[0] == "flip":
            src.append((src[spec[1]][0], not src[spec[1]][1]))
            pool.add_flipped(spec[1], spec[2])
        else:
            im = rng.randint(0, 256, size=(spec[0], spec[1], 3)).astype(np.uint8)
            src.append((im, False))
            pool.add(torch.from_numpy(im).to(dev) if len(src) % 2 == 0 else im, spec[2])
    return pool.freeze(), src


def per_image(dev, pool, src, plan, supports, target, ws, S, nb):
    """the per-image path into fresh holders + the all-class boxes, from the plan's host records"""
    from dana_amd import pipeline as PL
    B = max(plan.batch, 1)
    H, W = plan.holder_hw if plan.holder_hw is not None else (1, 1)
    hold = PL.EpisodeHolders(B, 1, ws, H, W, dev, support_size=S, max_num_box=nb)
    prepared = {}

    def prep(row):
        if row not in prepared:
            prepared[row] = PL.prep_im_for_blob(torch.from_numpy(src[row][0]).to(dev), MEANS, target, flipped=src[row][1])
        return prepared[row]

    for b, q in enumerate(plan.queries):
        im, s = prep(q["row"])
        hold.put_query(b, im, s, q["y_s"], q["x_s"], q["copy_h"], q["copy_w"])
    for n, (row, box) in enumerate(supports):
        im, s = prep(row)
        sb = (np.array(box, dtype=np.float32) * s).astype(np.int16)  # fs_loader.py:120, as test_gpu_pipeline.py does
        hold.put_support(n // ws, n % ws, im, sb)
    all_cls = torch.zeros((B, nb, 5), device=dev)
    if plan.batch:
        fs, n_fs, al, n_al = plan.boxes_numpy(pool, nb)
        for b in range(plan.batch):
            hold.put_boxes(b, fs[b][:n_fs[b]])
        all_cls = torch.from_numpy(al).to(dev)
    return hold, all_cls


def same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, i
        if not torch.equal(a, b):
            d = (a.double() - b.double()).abs()
            raise AssertionError("tensor %d differs at %d of %d elements, max |diff| %.3e" % (i, int((a != b).sum()), a.numel(), float(d.max())))


QUERY_CASES = {
    # target 48 into 48 x 64: the three source sizes. 5x7 upscaled 9.6x, its crop ending at the last prepared column (7 + 60
    # = 67) and padded in x; the flipped 37x53 cropped to its last column; 64x48 at scale 1, the top-left 48 x 48 (ratio 1)
    "up_crop_flip": (48, (48, 64), [dict(row=0, ratio=1.25, pos_cls=2, need_crop=True, crop_start=7, order=[1, 0]),
                                    dict(row=3, ratio=1.25, pos_cls=1, need_crop=True, crop_start=9),
                                    dict(row=2, ratio=1.0, pos_cls=1, order=[2, 0, 1])]),
    # target 32 into 48 x 64: downscales. 37x53 -> 32 x 46 padded on both axes; 64x48 -> 43 x 32; the flipped twin's square
    "down_pad_both": (32, (48, 64), [dict(row=1, ratio=1.4, pos_cls=1), dict(row=2, ratio=0.75, pos_cls=1),
                                     dict(row=3, ratio=1.0, pos_cls=2)]),
    # B = 1: a height crop ending at the last prepared row (4 + 60 = 64) whose copy window IS the holder
    "one_equal_holder": (48, (60, 48), [dict(row=2, ratio=0.8, pos_cls=1, need_crop=True, crop_start=4)]),
}


@pytest.mark.parametrize("name", sorted(QUERY_CASES))
def test_queries_equal_the_per_image_path(dev, name):
    from dana_amd import pipeline as PL
    target, hw, queries = QUERY_CASES[name]
    pool, src = make_pool(dev, SMALL)
    plan = PL.plan_episode(pool, queries, holder_hw=hw, target_size=target)
    hold = PL.EpisodeHolders(len(queries), 1, 0, hw[0], hw[1], dev, support_size=32, max_num_box=4)
    for t in hold.tensors()[:4]:
        t.fill_(7)  # whatever was there must go
    asm = PL.EpisodeAssembler(pool, hold, pixel_means=MEANS)
    out = asm.assemble(plan)  # way * shot == 0: the query-only form
    assert [t.data_ptr() for t in out[:5]] == [t.data_ptr() for t in hold.tensors()]
    ref, ref_all = per_image(dev, pool, src, plan, [], target, 0, 32, 4)
    same(out, ref.tensors() + (ref_all,))
    assert torch.equal(asm.all_cls_num_boxes.cpu(), torch.from_numpy(plan.boxes_numpy(pool, 4)[3]))
    assert float(out[0].abs().max()) > 1 and int(out[3].sum()) > 0  # (not a comparison of zeros)


SUPPORTS = [(1, (53, 5, 54.5, 36)),   # at the right border: limited to ONE prepared column (cw == 1)
            (0, (0, 0, 2, 2)),        # the top-left corner of the 5 x 7 image
            (1, (0, 0, 53, 37)),      # the whole image: rh < target
            (2, (2, 2, 40, 60)),      # rw < target
            (3, (22, 4, 49, 20)),     # a flipped source row
            (2, (30, 40, 47, 63))]    # the bottom-right corner


@pytest.mark.parametrize("ws,target", [(1, 48), (6, 48), (6, 32)])
def test_supports_equal_the_per_image_path(dev, ws, target):
    from dana_amd import pipeline as PL
    pool, src = make_pool(dev, SMALL)
    sups = SUPPORTS[4:5] if ws == 1 else SUPPORTS
    q = [dict(row=1, ratio=1.0, pos_cls=1)]
    plan = PL.plan_episode(pool, q, sups, holder_hw=(48, 64), target_size=target, support_size=32)
    if ws == 6:
        s = plan.supports
        assert s[0]["cw"] == 1 and s[2]["rh"] < 32 and s[3]["rw"] < 32 and (s[1]["x_min"], s[1]["y_min"]) == (0, 0)
        assert (s[5]["x_max"], s[5]["y_max"]) == (s[5]["ow"] - 1, s[5]["oh"] - 1)
    hold = PL.EpisodeHolders(1, 1, ws, 48, 64, dev, support_size=32, max_num_box=4)
    hold.support_ims.fill_(7)
    out = PL.EpisodeAssembler(pool, hold, pixel_means=MEANS).assemble(plan)
    ref, ref_all = per_image(dev, pool, src, plan, sups, target, ws, 32, 4)
    same(out, ref.tensors() + (ref_all,))
    assert all(float(out[4][0, n].abs().max()) > 1 for n in range(ws))


def _run_boxes(dev, boxes, order, im_scale, x_s, y_s, clamp_x, clamp_y, pos_cls, mx):
    """dana_episode_boxes for one image whose record carries exactly these numbers"""
    from dana_amd import pipeline as PL
    from dana_amd._lib import lib
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 5)
    pool = PL.ImagePool(dev)
    pool.add(np.zeros((4, 4, 3), dtype=np.uint8), boxes)
    pool.freeze()
    plan = PL.plan_episode(pool, [dict(row=0, ratio=1.0, pos_cls=pos_cls, order=order)], holder_hw=(4, 4), target_size=4)
    w = plan.words
    w[PL.Q_SCALE:PL.Q_SCALE + 2].view(np.float64)[0] = im_scale
    w[PL.Q_YS], w[PL.Q_XS], w[PL.Q_CLAMP_X], w[PL.Q_CLAMP_Y] = y_s, x_s, clamp_x, clamp_y
    d_plan = torch.from_numpy(w).to(dev)
    fs = torch.full((1, mx, 5), 7.0, device=dev)
    al = torch.full((1, mx, 5), 7.0, device=dev)
    n_fs = torch.full((1,), -1, dtype=torch.long, device=dev)
    n_al = torch.full((1,), -1, dtype=torch.long, device=dev)
    lib().call("dana_episode_boxes", pool.d_boxes.data_ptr(), len(pool.boxes), pool.d_meta.data_ptr(), 1, d_plan.data_ptr(),
               int(w.size), 0, 1, mx, fs.data_ptr(), n_fs.data_ptr(), al.data_ptr(), n_al.data_ptr(),
               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return fs[0].cpu().numpy(), int(n_fs), al[0].cpu().numpy(), int(n_al)


def _many_boxes():
    """150 boxes (three passes of the wavefront), a third of them degenerate, two classes, shuffled, cut at 50"""
    rng = np.random.RandomState(5)
    b = np.zeros((150, 5), dtype=np.float32)
    b[:, 0:2] = rng.randint(0, 200, size=(150, 2))
    b[:, 2:4] = b[:, 0:2] + rng.randint(0, 3, size=(150, 2)) * 17
    b[:, 4] = rng.randint(1, 3, size=150)
    return (b, rng.permutation(150), 600.0 / 375.0, 30, 0, 299, -1, 2, 50)


BOX_ARGS = dict({k: v[0] for k, v in box_cases().items()},
                **{"150 boxes": _many_boxes(),
                   "double product": ([[9, 9, 18, 13, 1]], [0], 600.0 / 375.0, 0, 0, -1, -1, 1, 1)})


@pytest.mark.parametrize("name", sorted(BOX_ARGS))
def test_boxes_equal_the_numpy_restatement(dev, name):
    from dana_amd import pipeline as PL
    args = BOX_ARGS[name]
    want = PL.episode_boxes_numpy(np.asarray(args[0], dtype=np.float32), *args[1:])
    got = _run_boxes(dev, *args)
    print(name, "num_boxes", got[1], got[3], "expected", want[1], want[3])
    assert got[1] == want[1] and got[3] == want[3]
    assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()
    if name == "double product":
        assert float(got[0][0, 0]) == 14.399999618530273
    if name == "150 boxes":
        assert want[1] > 10 and want[3] == 50


def test_plans_in_flight_and_stale_data(dev):
    """A then B with no synchronise between them, B smaller in every respect; each stream-ordered clone equals its own
    per-image result, so B's upload did not reach A's launches and nothing A wrote survives B"""
    from dana_amd import pipeline as PL
    pool, src = make_pool(dev, SMALL)
    hold = PL.EpisodeHolders(2, 1, 2, 48, 64, dev, support_size=32, max_num_box=4)
    asm = PL.EpisodeAssembler(pool, hold, pixel_means=MEANS)
    sup_a = [SUPPORTS[2], SUPPORTS[5], SUPPORTS[4], SUPPORTS[1]]
    sup_b = [SUPPORTS[0], SUPPORTS[3], SUPPORTS[0], SUPPORTS[0]]
    plan_a = PL.plan_episode(pool, [dict(row=1, ratio=1.25, pos_cls=1, need_crop=True, crop_start=3),
                                    dict(row=2, ratio=1.0, pos_cls=1)], sup_a, holder_hw=(48, 64), target_size=48, support_size=32)
    plan_b = PL.plan_episode(pool, [dict(row=2, ratio=0.75, pos_cls=2, order=[1]), dict(row=0, ratio=1.4, pos_cls=2, order=[0])],
                             sup_b, holder_hw=(48, 64), target_size=32, support_size=32)
    for qa, qb in zip(plan_a.queries, plan_b.queries):
        assert qb["copy_h"] <= qa["copy_h"] and qb["copy_w"] < qa["copy_w"] and len(qb["order"]) < len(qa["order"])
    for sa, sb in zip(plan_a.supports, plan_b.supports):
        assert sb["rw"] * sb["rh"] < sa["rw"] * sa["rh"]
    got_a = [t.clone() for t in asm.assemble(plan_a)]
    got_b = [t.clone() for t in asm.assemble(plan_b)]
    got_b2 = [t.clone() for t in asm.assemble(plan_b)]  # the first buffer comes round again
    torch.cuda.synchronize()
    ref_a, all_a = per_image(dev, pool, src, plan_a, sup_a, 48, 2, 32, 4)
    ref_b, all_b = per_image(dev, pool, src, plan_b, sup_b, 32, 2, 32, 4)
    same(got_a, ref_a.tensors() + (all_a,))
    same(got_b, ref_b.tensors() + (all_b,))
    same(got_b2, got_b)
    assert int(got_b[3].sum()) < int(got_a[3].sum())
    with pytest.raises(ValueError, match="not for these holders"):
        asm.assemble(PL.plan_episode(pool, [dict(row=2, ratio=1.0, pos_cls=1)], holder_hw=(48, 64), target_size=48))


def test_reference_sizes_feed_the_model(dev):
    """bs 4, way 2, shot 3 at the reference's sizes: 375x500 and 480x333 sources at target 600, 320 x 320 supports. One
    holder takes both shapes at ratio 1 (pad_plan: the top-left 600 x 600 of 600x800 and of 865x600). Equal to the per-image
    path, and one train-mode forward from either gives the same 8-tuple: the new-path twin of
    test_episode_holders_feed_the_model."""
    import dana_amd
    from dana_amd import pipeline as PL, synthetic as S
    specs = [(375, 500, [[30, 40, 200, 300, 1], [250, 100, 480, 360, 2], [9, 9, 18, 13, 1]]),
             (480, 333, [[20, 30, 300, 400, 2], [100, 200, 320, 470, 1]]),
             ("flip", 0, [[299, 40, 469, 300, 1], [19, 100, 249, 360, 2]]),
             (375, 500, [[60, 50, 400, 330, 1]])]
    pool, src = make_pool(dev, specs, seed=8)
    queries = [dict(row=0, ratio=1.0, pos_cls=1, order=[2, 0, 1]), dict(row=1, ratio=1.0, pos_cls=2),
               dict(row=2, ratio=1.0, pos_cls=2, order=[1, 0]), dict(row=3, ratio=1.0, pos_cls=1)]
    boxes = [(0, (30, 40, 200, 300)), (1, (100, 200, 320, 470)), (2, (299, 40, 469, 300)),
             (3, (60, 50, 400, 330)), (0, (250, 100, 480, 360)), (1, (20, 30, 300, 400))]
    sups = [boxes[(b + k) % 6] for b in range(4) for k in range(6)]
    oh, ow, ch, cw = PL.pad_plan(600, 800, 1.0)
    assert (oh, ow) == (600, 600) == PL.pad_plan(865, 600, 1.0)[:2]
    plan = PL.plan_episode(pool, queries, sups, holder_hw=(oh, ow))
    hold = PL.EpisodeHolders(4, 2, 3, oh, ow, dev)
    out = PL.EpisodeAssembler(pool, hold, pixel_means=MEANS).assemble(plan)
    ref, ref_all = per_image(dev, pool, src, plan, sups, 600, 6, 320, hold.gt_boxes.size(1))
    same(out, ref.tensors() + (ref_all,))
    assert out[3].tolist() == [2, 1, 1, 1] and float(out[1][1, 2]) == np.float32(600.0 / 333.0)
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=2, shot=3, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=4, profile="test"))
    m.to(dev).train()
    res = []
    for tensors in (out[:5], ref.tensors()):
        np.random.seed(11)
        with torch.no_grad():
            res.append(m(*tensors))
    torch.cuda.synchronize()
    assert len(res[0]) == len(res[1]) == 8
    same([torch.as_tensor(t) for t in res[0]], [torch.as_tensor(t) for t in res[1]])
    assert all(torch.isfinite(torch.as_tensor(t).float()).all() for t in res[0])


def test_support_crops_feed_the_bank(dev):
    """support_crops -> encode_support_bank: the bank, and a train-mode forward from one of its episodes, equal those of the
    bank encoded from the per-image crops"""
    from test_gpu_support_bank import _build, _inputs
    from dana_amd import pipeline as PL
    specs = [(90, 120, []), (120, 100, []), ("flip", 0, [])]
    pool, src = make_pool(dev, specs, seed=3)
    sups = [(0, (10, 8, 70, 60)), (1, (20, 30, 80, 100)), (2, (5, 5, 115, 85)), (0, (40, 10, 60, 80)), (1, (0, 0, 99, 119)),
            (2, (60, 20, 119, 50))]
    records = PL.plan_episode(pool, (), sups, target_size=192)
    asm = PL.EpisodeAssembler(pool, pixel_means=MEANS)
    crops = asm.support_crops(records)
    assert tuple(crops.shape) == (6, 3, 320, 320)
    ref, _ = per_image(dev, pool, src, records, sups, 192, 6, 320, 1)
    assert torch.equal(crops, ref.support_ims[0])
    into = torch.full_like(crops, 7)
    assert asm.support_crops(records, out=into) is into and torch.equal(into, crops)
    m, _ = _build("DAnA", 3, dev, 1, use_BA_block=True)
    bank, bank_ref = m.encode_support_bank(crops), m.encode_support_bank(ref.support_ims[0].clone())
    assert torch.equal(bank.map_pe, bank_ref.map_pe) and torch.equal(bank.pool_pe, bank_ref.pool_pe)
    index = np.array([[0, 3], [4, 2]])
    inputs = _inputs(dev, 1)[:4]
    res = []
    for bk in (bank, bank_ref):
        np.random.seed(33)
        with torch.no_grad():
            res.append(m(*inputs, bk.episode(index)))
    torch.cuda.synchronize()
    same([torch.as_tensor(t) for t in res[0]], [torch.as_tensor(t) for t in res[1]])
    with pytest.raises(ValueError, match="supports only"):
        asm.support_crops(PL.plan_episode(pool, [dict(row=0, ratio=1.0, pos_cls=1)], holder_hw=(192, 192), target_size=192))
