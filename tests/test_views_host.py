"""CPU suite: view ensembles (flip and multi-scale testing merged on the device). `postprocess.fold_views_numpy` -- the
restatement test_gpu_views.py compares csrc/views.hip against -- on hand-worked rows of a 100 x 60 frame, `pipeline.plan_views`
against `_plan_query`, the margins of exactly the chained cases the GPU file runs (tests/views_cases.py), and the argument
errors of dana_detect_fold_views, which need no GPU."""
import ctypes

import numpy as np
import pytest

import views_cases as VC
from dana_amd import _lib, pipeline as PL, postprocess as PP

INF = np.inf
FRAME = [100.0, 60.0]  # fw, fh: wm1 = 99, hm1 = 59


def _fold1(rows, flip=0, lo=-INF, hi=INF, frame=FRAME):
    t = np.asarray([list(frame) + [flip, lo, hi]], np.float32)
    r = PP.fold_views_numpy([np.asarray(rows, np.float32).reshape(-1, 5)], t, 1, 1)
    assert r["counts"].dtype == np.int32 and r["counts"].tolist() == [len(r["dets"][0])] and r["source"].tolist() == [0]
    assert r["dets"][0].dtype == np.float32 and r["src_row"][0].dtype == np.int32
    return r["dets"][0], r["src_row"][0]


def test_flip_is_wm1_minus_x_and_an_involution():
    d, _ = _fold1([[10, 5, 30, 20, .9], [0, 0, 99, 59, .5]], flip=1)
    assert d.tolist() == [[69, 5, 89, 20, np.float32(.9)], [0, 0, 99, 59, .5]]
    rng = np.random.RandomState(0)
    x1, y1 = rng.uniform(0, 60, 50), rng.uniform(0, 40, 50)
    # quarter-pixel coordinates: 99 - x is exact, so mirroring twice returns the input's own bits
    boxes = (np.round(np.stack((x1, y1, x1 + rng.uniform(1, 39, 50), y1 + rng.uniform(1, 19, 50)), 1) * 4) / 4).astype(np.float32)
    rows = np.concatenate((boxes, rng.uniform(0, 1, (50, 1)).astype(np.float32)), 1)
    once, src = _fold1(rows, flip=1)
    assert src.tolist() == list(range(50)) and not np.array_equal(once, rows)
    assert np.array_equal(once[:, 0], np.float32(99) - rows[:, 2]) and np.array_equal(once[:, 2], np.float32(99) - rows[:, 0])
    twice, _ = _fold1(once, flip=1)
    assert np.array_equal(twice.view(np.int32), rows.view(np.int32))
    # one rounding: wm1 - x, not (fw - x) - 1. On a 65-pixel frame the two differ: 64 - 0.3 lies below 64, where floats
    # are twice as dense as at 65 - 0.3
    x = np.float32(0.3)
    assert np.float32(64) - x != (np.float32(65) - x) - np.float32(1)
    d, _ = _fold1([[0.3, 0, 0.3, 0, .5]], flip=1, frame=(65.0, 60.0))
    assert d[0, 0] == np.float32(64) - x == d[0, 2]


def test_frame_test_and_clip():
    rows = [[99, 10, 120, 20, .9],    # x1 == wm1: touches the last column, stays, clipped to one column
            [100, 10, 120, 20, .8],   # x1 == wm1 + 1: outside
            [90, 50, 110, 70, .7],    # straddles the right and the bottom edge
            [-30, -20, -1, 5, .6],    # x2 < 0: outside
            [-30, -20, 0, 0, .5],     # x2 == 0, y2 == 0: touches the first pixel
            [10, 60, 20, 70, .4],     # y1 == hm1 + 1: outside
            [10, 59, 20, 70, .3]]     # y1 == hm1: stays
    d, src = _fold1(rows)
    assert src.tolist() == [0, 2, 4, 6]
    assert d[:, :4].tolist() == [[99, 10, 99, 20], [90, 50, 99, 59], [0, 0, 0, 0], [10, 59, 20, 59]]
    assert d[:, 4].tolist() == [np.float32(s) for s in (.9, .7, .5, .3)]  # the score is copied


def test_nan_rows_are_dropped_and_the_order_is_the_input_order():
    nan = np.nan
    rows = [[1, 1, 5, 5, .9], [nan, 1, 5, 5, .8], [1, nan, 5, 5, .7], [2, 2, 6, 6, .6], [1, 1, nan, 5, .5], [1, 1, 5, nan, .4],
            [3, 3, 7, 7, .3]]
    for flip in (0, 1):
        d, src = _fold1(rows, flip=flip)
        assert src.tolist() == [0, 3, 6] and d[:, 4].tolist() == [np.float32(s) for s in (.9, .6, .3)]
    # a NaN score is not a coordinate: the row stays and the score's bits are copied
    d, src = _fold1([[1, 1, 5, 5, nan]])
    assert src.tolist() == [0] and np.isnan(d[0, 4])


def test_area_window_is_closed_below_and_open_above():
    rows = [[0, 0, 9, 9, .9], [0, 0, 9, 10, .8], [0, 0, 10, 10, .7], [0, 0, 3, 3, .6]]  # areas 100, 110, 121, 16
    assert _fold1(rows, lo=100, hi=121)[1].tolist() == [0, 1]   # area == lo stays, area == hi goes
    assert _fold1(rows, lo=101, hi=INF)[1].tolist() == [1, 2]
    assert _fold1(rows, lo=-INF, hi=100)[1].tolist() == [3]
    assert _fold1(rows)[1].tolist() == [0, 1, 2, 3]
    # the area is the CLIPPED box's: 20 x 20 hanging over the corner leaves 10 x 10
    assert _fold1([[90, 50, 109, 69, .5]], lo=100, hi=101)[1].tolist() == [0]


def test_layout_transposition_for_b2_v3_c2():
    B, V, C = 2, 3, 2
    lists = [np.asarray([[p, p, p + 1, p + 1, .5]] * (p + 1), np.float32) for p in range(B * V * C)]
    table = np.asarray([FRAME + [0, -INF, INF]] * (B * V), np.float32)
    r = PP.fold_views_numpy(lists, table, V, C)
    # q = (i * C + c) * V + v  <-  p = (i * V + v) * C + c
    assert r["source"].tolist() == [0, 2, 4, 1, 3, 5, 6, 8, 10, 7, 9, 11]
    assert r["counts"].tolist() == [p + 1 for p in r["source"]]
    for q, p in enumerate(r["source"]):
        assert np.array_equal(r["dets"][q], lists[p]) and r["src_row"][q].tolist() == list(range(p + 1))
    # the table row is the VIEW's (i * V + v), whatever the class slot: mirror view 1 of image 1 only
    table[1 * V + 1, 2] = 1
    r = PP.fold_views_numpy(lists, table, V, C)
    for q, p in enumerate(r["source"]):
        mirrored = p in (8, 9)
        assert (r["dets"][q][0, 0] == 99 - (p + 1)) if mirrored else (r["dets"][q][0, 0] == p), (q, p)
    with pytest.raises(ValueError, match="fold_views_numpy"):
        PP.fold_views_numpy(lists[:5], table, V, C)
    with pytest.raises(ValueError, match="fold_views_numpy"):
        PP.fold_views_numpy(lists, table[:5], V, C)


# ---- plan_views ---------------------------------------------------------------------------------------------------------

def _im(h, w):
    return np.zeros((h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def pool():
    p = PL.ImagePool()
    p.add(_im(96, 128), [[1, 1, 40, 30, 1]])      # row 0
    p.add(_im(120, 90), [])                       # row 1
    p.add_flipped(0, [[87, 1, 126, 30, 1]])       # row 2: twin of 0
    p.add_flipped(1, [])                          # row 3: twin of 1
    p.add(_im(96, 128), [])                       # row 4: the size of row 0, another frame
    return p.freeze()


def test_pool_tells_frames_and_flipped_bits(pool):
    assert [pool.frame_of(r) for r in range(5)] == [0, 1, 0, 1, 2]
    assert pool.meta[:, 2].tolist() == [0, 0, 1, 1, 0]


def test_plan_views_order_scales_and_table(pool):
    scales = (64, 96, 48)
    plan, views = PL.plan_views(pool, [(0, 2), (1, 3)], scales=scales, flip=True)
    assert (views.n_images, views.views) == (2, 6) and plan.batch == 12 and plan.n_supports == 0
    assert views.table.dtype == np.float32 and views.table.shape == (12, 5)
    assert plan.words.dtype == np.int32 and plan.words.size == 12 * PL.EP_QWORDS
    f64 = plan.words.view(np.float64)
    for i, (row, twin) in enumerate([(0, 2), (1, 3)]):
        h, w = int(pool.meta[row, 0]), int(pool.meta[row, 1])
        for s, scale in enumerate(scales):
            ref = PL._plan_query(pool, dict(row=row, ratio=1.0, pos_cls=0), (10 ** 6, 10 ** 6), scale)
            for f in (0, 1):
                v = s * 2 + f  # v = s * F + f
                b = i * 6 + v
                q, o = plan.queries[b], b * PL.EP_QWORDS
                assert q["view"] == v and q["row"] == (twin if f else row) == plan.words[o + PL.Q_ROW] == views.rows[b]
                assert q["im_scale"] == ref["im_scale"] == scale / min(h, w) == f64[(o + PL.Q_SCALE) // 2] == views.scales[b]
                assert f64[(o + PL.Q_INV) // 2] == 1.0 / ref["im_scale"]
                assert (plan.words[o + PL.Q_OH], plan.words[o + PL.Q_OW]) == (ref["oh"], ref["ow"]) == (q["oh"], q["ow"])
                # the whole prepared image at the top-left corner; no clamp; no boxes
                assert plan.words[o + PL.Q_YS:o + PL.Q_YS + 4].tolist() == [0, 0, ref["oh"], ref["ow"]]
                assert plan.words[o + PL.Q_CLAMP_X:o + PL.Q_CLAMP_X + 2].tolist() == [-1, -1] and plan.words[o + PL.Q_NORDER] == 0
                # the table carries the FRAME's size, not the prepared one, and the row's flipped bit
                assert views.table[b].tolist() == [w, h, f, -INF, INF]
    # the default holder is the maximum prepared size over all views: 96x128 at 96 -> 96 x 128, 120x90 at 96 -> 128 x 96
    assert plan.holder_hw == (128, 128) == PL.views_holder_hw(pool, [(0, 2), (1, 3)], scales)
    assert PL.views_holder_hw(pool, [0], (64,)) == (64, 85) and PL.views_holder_hw(pool, [1], (64,)) == (85, 64)
    # without flip: V = len(scales), plain rows; a twin row alone is a mirrored view
    plan1, v1 = PL.plan_views(pool, [1, 2], scales=(64,), area_ranges=[(0, 1000)])
    assert (v1.n_images, v1.views, plan1.batch) == (2, 1, 2) and plan1.holder_hw == (85, 85)
    assert v1.table.tolist() == [[90, 120, 0, 0, 1000], [128, 96, 1, 0, 1000]]
    # area windows are per scale
    _, v2 = PL.plan_views(pool, [(0, 2)], scales=(48, 96), flip=True, area_ranges=[(400, INF), (0, 400)])
    assert v2.table[:, 3:].tolist() == [[400, INF], [400, INF], [0, 400], [0, 400]]
    # a larger holder is fine and kept
    assert PL.plan_views(pool, [0], scales=(64,), holder_hw=(100, 200))[0].holder_hw == (100, 200)
    # plan_episode packs through the same helper: its words are unchanged by the refactoring's look
    pe = PL.plan_episode(pool, [dict(row=0, ratio=1.0, pos_cls=1)], holder_hw=(128, 128), target_size=64)
    assert pe.words[PL.Q_NORDER] == 1 and pe.words.size == PL.EP_QWORDS + 1


def test_plan_views_refusals(pool):
    open_pool = PL.ImagePool()
    open_pool.add(_im(8, 8), [])
    with pytest.raises(RuntimeError, match="freeze"):
        PL.plan_views(open_pool, [0], scales=(8,))
    with pytest.raises(ValueError, match="flip=True needs"):
        PL.plan_views(pool, [0], scales=(64,), flip=True)
    with pytest.raises(ValueError, match="need flip=True"):
        PL.plan_views(pool, [(0, 2)], scales=(64,))
    with pytest.raises(ValueError, match="different frames"):
        PL.plan_views(pool, [(0, 3)], scales=(64,), flip=True)
    with pytest.raises(ValueError, match="different frames"):  # the same size is not the same frame
        PL.plan_views(pool, [(0, 4)], scales=(64,), flip=True)
    with pytest.raises(ValueError, match="both have flipped = 0"):
        PL.plan_views(pool, [(0, 0)], scales=(64,), flip=True)
    with pytest.raises(ValueError, match="larger than the holder"):
        PL.plan_views(pool, [0], scales=(64, 96), holder_hw=(64, 85))
    with pytest.raises(ValueError, match="area ranges"):
        PL.plan_views(pool, [0], scales=(64, 96), area_ranges=[(0, 1)])
    with pytest.raises(ValueError, match="scales"):
        PL.plan_views(pool, [0], scales=())
    with pytest.raises(IndexError):
        PL.plan_views(pool, [7], scales=(64,))

    class _Dev:  # stands for a device tensor where there is no device: the check reads `is_cuda`
        is_cuda = True
    with pytest.raises(ValueError, match="device tensor"):
        PL.plan_views(pool, [_Dev()], scales=(64,))
    with pytest.raises(ValueError, match="device tensor"):
        PL.plan_views(pool, [(0, _Dev())], scales=(64,), flip=True)
    with pytest.raises(ValueError, match="device tensor"):
        PL.plan_views(pool, [0], scales=(_Dev(),))


# ---- the chained cases of the GPU file ----------------------------------------------------------------------------------

def test_margins_of_the_chained_gpu_cases():
    """what makes test_gpu_views.py's chained comparisons meaningful: on the FOLDED lists of every case it runs, the float64
    merge's suppression margin and -- under gaussian or with voting -- the restatement's pick and drop margins hold, as
    test_soft_merge_host.py asserts them for the soft-merge suite; and the fold really un-mirrors onto the clusters"""
    import soft_merge_cases as C
    checked = 0
    for name in VC.CHAINED:
        lists, table, B, V, Cn = VC.chained_inputs(name)
        folded = VC.folded_reference(name)
        assert int(folded["counts"].sum()) == sum(len(q) for q in lists) > 0  # nothing is dropped: the frame holds every box
        hard = PP.merge_numpy(folded["dets"], V, C.THR)
        assert hard["margin"] >= C.MARGIN, (name, hard["margin"])
        # half of the views were mirrored beforehand; folded, their boxes lie on the unmirrored clusters again
        clean = VC.chained_clean(name)
        for q, p in enumerate(folded["source"]):
            assert np.abs(folded["dets"][q][:, :4] - clean[p][:, :4]).max(initial=0) <= 2e-3
        assert any(table[iv, 2] for iv in range(B * V)) and not all(table[iv, 2] for iv in range(B * V))
        assert int(hard["counts"].sum()) < int(folded["counts"].sum())  # the views overlap: the merge suppresses
        for method, vote in VC.CHAINED_RUNS:
            ref = VC.chained_reference(name, method, vote)
            if C.needs_margin(method, vote):
                m = ref["margin"]
                assert m["pick"] >= C.MARGIN and m["drop"] >= C.MARGIN, (name, method, vote, m)
                L = max(int(folded["counts"][l * V:(l + 1) * V].sum()) for l in range(B * Cn))
                assert method != "gaussian" or L <= 80, (name, L)
            checked += 1
    assert checked == len(VC.CHAINED) * 6


def test_fold_cases_cover_what_they_claim():
    lengths = set()
    for name, (B, V, C) in VC.FOLD_SHAPES.items():
        lists, table, packed, counts, offsets = VC.fold_inputs(name)
        assert len(lists) == B * V * C and table.shape == (B * V, VC.STRIDE)
        lengths |= set(int(c) for c in counts)
        ref = VC.fold_reference(name)
        kept = [int(ref["counts"][q]) for q in range(len(lists))]
        n_in = [int(counts[p]) for p in ref["source"]]
        if name == "b2v3c2":  # every drop pattern occurs
            pats = {"none": False, "all": False, "other": False}
            for q, p in enumerate(ref["source"]):
                if n_in[q] >= 2:
                    pats["none"] |= kept[q] == n_in[q]
                    pats["all"] |= kept[q] == 0
                    pats["other"] |= ref["src_row"][q].tolist() == list(range(0, n_in[q], 2))
            assert all(pats.values()), pats
        # lists are packed with gaps, at offsets that are no multiple of anything
        assert all(int(offsets[p + 1]) > int(offsets[p]) + int(counts[p]) for p in range(len(lists) - 1))
    assert lengths >= {0, 1, 63, 64, 65, 255, 256, 257, 1000}
    assert any(int(o) % 2 for o in VC.fold_inputs("b2v3c2")[4][1:])
    single = VC.fold_reference("b1v1c1")
    assert single["src_row"][0].tolist() == [0] and VC.fold_inputs("b1v1c1")[3].tolist() == [1000]  # only the first row stays
    last = VC.fold_reference("b1v2c1")
    assert last["src_row"][0].tolist() == [255] and last["src_row"][1].tolist() == [255, 511, 767]  # only the last row of a chunk


# ---- the C entry point without a GPU ------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_fold():
    protos = _lib.parse_header()
    assert "dana_detect_fold_views" in protos and hasattr(ctypes.CDLL(_lib.LIB_PATH), "dana_detect_fold_views")
    args = [a for _, a in protos["dana_detect_fold_views"][1]]
    assert args == ["dets_in", "counts_in", "offsets_in", "n_images", "views", "lists_per_view", "view_table", "view_stride",
                    "dets_out", "counts_out", "offsets_out", "src_row_out", "stream"]
    assert _lib.lib().query("dana_abi_version") == 1  # the change is additive


def test_fold_argument_errors_are_reported_without_a_gpu():
    L = _lib.lib()
    p, o = 16, 32  # (never dereferenced: every call below returns before its launch)
    call = lambda *a: L.call("dana_detect_fold_views", *a)  # noqa: E731
    for k in (0, 1, 2, 6, 8, 9, 10):  # every pointer but src_row_out, which may be null
        a = [p, p, p, 1, 2, 3, p, 5, o, p, p, None, None]
        a[k] = None
        with pytest.raises(_lib.DanaError, match="dana_detect_fold_views: null pointer"):
            call(*a)
    with pytest.raises(_lib.DanaError, match="view_stride 4 < 5"):
        call(p, p, p, 1, 2, 3, p, 4, o, p, p, p, None)
    with pytest.raises(_lib.DanaError, match="dets_out must not alias dets_in"):
        call(p, p, p, 1, 2, 3, p, 5, p, p, p, p, None)
    with pytest.raises(_lib.DanaError, match="bad shape"):
        call(p, p, p, -1, 2, 3, p, 5, o, p, p, p, None)
    with pytest.raises(_lib.DanaError, match="lists"):
        call(p, p, p, 1 << 20, 1 << 10, 4, p, 5, o, p, p, p, None)
    # zero size: returns before anything is looked at, whichever factor is zero
    for shape in ((0, 2, 3), (1, 0, 3), (1, 2, 0)):
        call(None, None, None, *shape, None, 0, None, None, None, None, None)


def test_python_argument_errors_come_before_any_c_call():
    class _CD(list):
        packed = counts = offsets = layout_dev = None
        num_classes = 2
    views = PL.ViewSet(2, 3, np.zeros((6, 5), np.float32), np.ones(6), np.zeros(6))
    with pytest.raises(ValueError, match="5 images in the detections, but 2 images x 3 views"):
        PP.fold_views(_CD([[]] * 5), views)
    with pytest.raises(ValueError, match="method"):
        PP.ensemble_views(None, views, method="soft")
    with pytest.raises(ValueError, match="vote_thresh"):
        PP.ensemble_views(None, views, vote_thresh=1.5)
    with pytest.raises(ValueError, match="linear"):
        PP.ensemble_views(None, views, nms_thresh=None, method="linear")
