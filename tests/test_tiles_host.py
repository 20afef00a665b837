"""CPU suite: tiled inference (overlapping tiles folded and merged on the device). `pipeline.tile_windows` and its coverage
guarantee by brute force, `pipeline.plan_tiles` on one hand-worked frame, `postprocess.fold_tiles_numpy` -- the restatement
test_gpu_tiles.py compares csrc/views.hip against -- on hand-worked rows, the margins of exactly the chained cases the GPU
file runs (tests/tiles_cases.py), and the argument errors of dana_detect_fold_tiles, which need no GPU."""
import ctypes

import numpy as np
import pytest

import tiles_cases as TC
import views_cases as VC
from dana_amd import _lib, pipeline as PL, postprocess as PP

INF = np.inf


# ---- the window rule ----------------------------------------------------------------------------------------------------

def _degenerate(L, n, o, m):
    if n == 1:
        return False
    T = -(-(L + (n - 1) * o) // n)
    return T > L or L - T < n - 1 or o - 2 * m < 1


def test_windows_start_at_0_end_at_L_and_overlap():
    assert PL.tile_windows(96, 2, 16, 2) == ([0, 40], 56) and PL.tile_windows(128, 2, 16, 2) == ([0, 56], 72)
    assert PL.tile_windows(1333, 1, 64, 4) == ([0], 1333)  # one tile is the axis, whatever overlap and margin
    assert PL.tile_windows(7, 1, 0, 5) == ([0], 7)
    assert PL.tile_windows(1000, 3, 64, 4) == ([0, 312, 624], 376)  # ceil(1128 / 3) = 376; k * 624 // 2
    assert PL.tile_windows(1001, 4, 17, 0) == ([0, 246, 492, 738], 263)  # ceil(1052 / 4); k * 738 // 3
    checked = 0
    for L in list(range(20, 61)) + [600, 1333]:
        for n in range(2, 5):
            for o, m in ((5, 1), (16, 3), (17, 0)):
                if _degenerate(L, n, o, m):
                    continue
                starts, T = PL.tile_windows(L, n, o, m)
                assert T == -(-(L + (n - 1) * o) // n) and len(starts) == n
                assert starts == [(k * (L - T)) // (n - 1) for k in range(n)]
                assert starts[0] == 0 and starts[-1] + T == L
                assert all(b > a and a + T - b >= o for a, b in zip(starts, starts[1:])), (L, n, o, m)
                checked += 1
    assert checked > 300


def test_coverage_guarantee_by_brute_force():
    """every integer interval [a, b] of the axis with b - a <= o - 2m lies in a window where it keeps m from every interior
    side: the placement the seam rule of the fold lets through in at least one tile"""
    placements = 0
    for L in list(range(20, 61)) + [600, 1333]:
        for n in range(1, 5):
            for o, m in ((5, 1), (16, 3), (17, 0)):
                if _degenerate(L, n, o, m):
                    continue
                starts, T = PL.tile_windows(L, n, o, m)
                s = np.asarray(starts)[:, None, None]
                a = np.arange(L)[None, :, None]
                b = a + np.arange(0, o - 2 * m + 1)[None, None, :]  # b - a = 0 .. o - 2m
                ok = ((a >= s + m) | (s == 0)) & ((b <= s + T - 1 - m) | (s + T == L)) & (a >= s) & (b <= s + T - 1)
                valid = (b <= L - 1)[0]
                assert ok.any(0)[valid].all(), (L, n, o, m)
                placements += int(valid.sum())
    assert placements > 50000


def test_windows_that_cannot_be_are_refused():
    with pytest.raises(ValueError, match="windows of 36 on an axis of 30"):  # T > L: ceil((30 + 42) / 2)
        PL.tile_windows(30, 2, 42, 4)
    with pytest.raises(ValueError, match="5 tiles of 20 on an axis of 20 prepared pixels would coincide"):
        PL.tile_windows(20, 5, 20, 4)  # T == L: every window would be the whole axis
    with pytest.raises(ValueError, match="3 tiles of 29 on an axis of 30 prepared pixels would coincide"):
        PL.tile_windows(30, 3, 28, 4)  # L - T = 1 < n - 1 = 2
    with pytest.raises(ValueError, match=r"overlap 8 - 2 \* margin 4 < 1"):
        PL.tile_windows(600, 2, 8, 4)
    with pytest.raises(ValueError, match=r"overlap 0 - 2 \* margin 0 < 1"):
        PL.tile_windows(600, 3, 0, 0)
    assert PL.tile_windows(600, 2, 9, 4)[1] == 305  # o - 2m == 1 is the least that is allowed
    with pytest.raises(ValueError, match="tiles >= 1"):
        PL.tile_windows(600, 0, 64, 4)
    with pytest.raises(ValueError, match="margin >= 0"):
        PL.tile_windows(600, 2, 64, -1)


# ---- plan_tiles ---------------------------------------------------------------------------------------------------------

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


def test_plan_tiles_of_the_hand_worked_frame(pool):
    """96 x 128, grid (2, 2), scale 96 (im_scale 1: prepared pixels are frame pixels), overlap 16, margin 2, flipped twins and
    a full-frame view at 64. Rows: L = 96 -> T = ceil(112 / 2) = 56, starts 0, 40; columns: L = 128 -> T = 72, starts 0, 56."""
    plan, tiles = PL.plan_tiles(pool, [(0, 2)], grid=(2, 2), scale=96, overlap=16, margin=2, flip=True, full_frame=64)
    assert isinstance(tiles, PL.TileSet) and isinstance(tiles, PL.ViewSet)
    assert (tiles.n_images, tiles.views, plan.batch, plan.n_supports) == (1, 10, 10, 0)
    assert tiles.table.dtype == np.float32 and tiles.table.shape == (10, 13) and tiles.windows.dtype == np.int32
    # v = t * 2 + f: t = 0 the full frame, then the tiles row-major; f = 1 the twin
    assert tiles.rows.tolist() == [0, 2] * 5 and [q["view"] for q in plan.queries] == list(range(10))
    assert tiles.scales.tolist() == [64 / 96] * 2 + [1.0] * 8
    assert tiles.windows.tolist() == [[0, 0, 64, 85], [0, 0, 64, 85],          # the whole frame at 64: 64 x round(85.33)
                                      [0, 0, 56, 72], [0, 0, 56, 72],          # tile (0, 0)
                                      [0, 56, 56, 72], [0, 56, 56, 72],        # tile (0, 1)
                                      [40, 0, 56, 72], [40, 0, 56, 72],        # tile (1, 0)
                                      [40, 56, 56, 72], [40, 56, 56, 72]]      # tile (1, 1)
    want = [[0, 0, 128, 96, -INF, -INF, INF, INF],    # the full frame: no offset, its own size, no seam
            [0, 0, 72, 56, -INF, -INF, 69, 53],       # top left: seams at its right and bottom side
            [56, 0, 72, 56, 2, -INF, INF, 53],        # top right: left and bottom
            [0, 40, 72, 56, -INF, 2, 69, INF],        # bottom left: top and right
            [56, 40, 72, 56, 2, 2, INF, INF]]         # bottom right: left and top
    for v in range(10):
        # the twin's window is the same numbers in the mirrored frame; only its flipped bit differs
        assert tiles.table[v].tolist() == [128, 96, v % 2, -INF, INF] + want[v // 2], v
    assert plan.holder_hw == (64, 85) == PL.tiles_holder_hw(pool, [(0, 2)], (2, 2), 96, 16, 2, 64)
    assert PL.tiles_holder_hw(pool, [0], (2, 2), 96, 16, 2, None) == (56, 72)
    # the records: the window at the holder's corner, no clamp, no boxes; the full frame is plan_views' record
    ref_plan, _ = PL.plan_views(pool, [(0, 2)], scales=(64,), flip=True, holder_hw=(64, 85))
    same = [w for w in range(2 * PL.EP_QWORDS) if w % PL.EP_QWORDS != PL.Q_ORDER_OFF]  # (where the box orders would start)
    assert plan.words[same].tolist() == ref_plan.words[same].tolist()
    f64 = plan.words.view(np.float64)
    for b in range(2, 10):
        o = b * PL.EP_QWORDS
        assert plan.words[o + PL.Q_ROW] == (0, 2)[b % 2] and plan.words[o + PL.Q_NORDER] == 0
        assert f64[(o + PL.Q_SCALE) // 2] == 1.0 == f64[(o + PL.Q_INV) // 2]
        assert plan.words[o + PL.Q_YS:o + PL.Q_YS + 4].tolist() == tiles.windows[b].tolist()
        assert plan.words[o + PL.Q_CLAMP_X:o + PL.Q_CLAMP_X + 2].tolist() == [-1, -1]
        assert (plan.words[o + PL.Q_OH], plan.words[o + PL.Q_OW]) == (96, 128)  # the PREPARED frame, not the window
    assert tiles.table_dev("cpu").shape == (10, 13)


def test_plan_tiles_scales_offsets_once_and_takes_area_ranges(pool):
    # 120 x 90 at scale 135: im_scale 1.5, prepared 180 x 135; grid (2, 1): rows T = ceil(200 / 2) = 100, starts 0, 80
    plan, tiles = PL.plan_tiles(pool, [1, 3], grid=(2, 1), scale=135, overlap=20, margin=3, full_frame=None,
                                area_ranges=((900, INF), (0, 900)))
    assert (tiles.n_images, tiles.views, plan.batch) == (2, 2, 4) and plan.holder_hw == (100, 135)
    assert tiles.windows.tolist() == [[0, 0, 100, 135], [80, 0, 100, 135]] * 2
    f = np.float32
    for b, flip in ((0, 0), (2, 1)):  # row 3 alone is a mirrored image
        assert tiles.table[b].tolist() == [90, 120, flip, 0, 900, 0, 0, 90, f(100 / 1.5), -INF, -INF, INF, f(96 / 1.5)]
        assert tiles.table[b + 1].tolist() == [90, 120, flip, 0, 900, 0, f(80 / 1.5), 90, f(100 / 1.5), -INF, f(3 / 1.5), INF, INF]
    # one column of tiles: the x axis has no seam at all; a division in float64 rounded once is not float32 / float32
    _, t2 = PL.plan_tiles(pool, [0], grid=(1, 2), scale=100, overlap=16, margin=2, full_frame=96, area_ranges=((900, INF), (0, 900)))
    s = 100 / 96
    xs, T = PL.tile_windows(PL.cv_round(128 * s), 2, 16, 2)
    assert t2.table[0].tolist() == [128, 96, 0, 900, INF, 0, 0, 128, 96, -INF, -INF, INF, INF]
    assert t2.table[2].tolist() == [128, 96, 0, 0, 900, f(xs[1] / s), 0, f(T / s), f(100 / s), f(2 / s), -INF, INF, INF]
    assert t2.table[2, 5] == np.float32(np.float64(xs[1]) / np.float64(s))


def test_plan_tiles_refusals(pool):
    kw = dict(grid=(2, 2), scale=96, overlap=16, margin=2)
    with pytest.raises(ValueError, match="flip=True needs"):
        PL.plan_tiles(pool, [0], flip=True, **kw)
    with pytest.raises(ValueError, match="need flip=True"):
        PL.plan_tiles(pool, [(0, 2)], **kw)
    with pytest.raises(ValueError, match="different frames"):
        PL.plan_tiles(pool, [(0, 3)], flip=True, **kw)
    with pytest.raises(ValueError, match="different frames"):
        PL.plan_tiles(pool, [(0, 4)], flip=True, **kw)
    with pytest.raises(ValueError, match="both have flipped = 0"):
        PL.plan_tiles(pool, [(0, 0)], flip=True, **kw)
    with pytest.raises(ValueError, match="larger than the holder"):  # the full frame at 64 is 64 x 85
        PL.plan_tiles(pool, [0], full_frame=64, holder_hw=(64, 80), **kw)
    with pytest.raises(ValueError, match="larger than the holder"):  # a tile is 56 x 72
        PL.plan_tiles(pool, [0], full_frame=None, holder_hw=(55, 72), **kw)
    assert PL.plan_tiles(pool, [0], full_frame=None, holder_hw=(56, 72), **kw)[0].holder_hw == (56, 72)
    with pytest.raises(ValueError, match="would coincide"):
        PL.plan_tiles(pool, [0], grid=(2, 120), scale=96, overlap=16, margin=2)
    with pytest.raises(ValueError, match="need windows of"):
        PL.plan_tiles(pool, [0], grid=(2, 2), scale=96, overlap=200, margin=2)
    with pytest.raises(ValueError, match=r"overlap 4 - 2 \* margin 2 < 1"):
        PL.plan_tiles(pool, [0], grid=(2, 1), scale=96, overlap=4, margin=2)
    with pytest.raises(ValueError, match="grid"):
        PL.plan_tiles(pool, [0], grid=(0, 2), scale=96, overlap=16, margin=2)
    with pytest.raises(ValueError, match="area_ranges"):
        PL.plan_tiles(pool, [0], area_ranges=[(0, 1)], **kw)
    with pytest.raises(ValueError, match="positive"):
        PL.plan_tiles(pool, [0], grid=(1, 1), scale=0)
    with pytest.raises(IndexError):
        PL.plan_tiles(pool, [7], **kw)
    open_pool = PL.ImagePool()
    open_pool.add(_im(8, 8), [])
    with pytest.raises(RuntimeError, match="freeze"):
        PL.plan_tiles(open_pool, [0], grid=(1, 1), scale=8)

    class _Dev:  # stands for a device tensor where there is no device: the check reads `is_cuda`
        is_cuda = True
    with pytest.raises(ValueError, match="device tensor"):
        PL.plan_tiles(pool, [_Dev()], **kw)
    with pytest.raises(ValueError, match="device tensor"):
        PL.plan_tiles(pool, [0], grid=(1, 1), scale=_Dev())


# ---- fold_tiles_numpy on hand-worked rows -------------------------------------------------------------------------------

FRAME = [100.0, 60.0]  # fw, fh: wm1 = 99, hm1 = 59
MIDDLE = [30, 10, 50, 40, 2, 2, 47, 37]         # a 50 x 40 tile at (30, 10), four interior sides, margin 2
CORNER0 = [0, 0, 50, 40, -INF, -INF, 47, 37]    # the frame's top-left tile
CORNER1 = [50, 20, 50, 40, 2, 2, INF, INF]      # its bottom-right tile: 50 + 50 = 100, 20 + 40 = 60


def _fold1(rows, tile, flip=0, lo=-INF, hi=INF, frame=FRAME):
    t = np.asarray([list(frame) + [flip, lo, hi] + list(tile)], np.float32)
    r = PP.fold_tiles_numpy([np.asarray(rows, np.float32).reshape(-1, 5)], t, 1, 1)
    assert r["counts"].dtype == np.int32 and r["counts"].tolist() == [len(r["dets"][0])] and r["source"].tolist() == [0]
    assert r["dets"][0].dtype == np.float32 and r["src_row"][0].dtype == np.int32
    return r["dets"][0], r["src_row"][0]


def test_seam_rule_on_a_limit_and_a_quarter_pixel_inside_it():
    rows = [[2, 2, 20, 20, .9],        # x1 == lim_x1, y1 == lim_y1: stays
            [1.75, 2, 20, 20, .8],     # a quarter pixel into the left margin
            [10, 10, 47, 37, .7],      # x2 == lim_x2, y2 == lim_y2: stays
            [10, 10, 47.25, 37, .6],   # ... into the right margin
            [10, 10, 47, 37.25, .5],   # ... the bottom margin
            [2, 1.75, 20, 20, .4]]     # ... the top margin
    d, src = _fold1(rows, MIDDLE)
    assert src.tolist() == [0, 2]
    assert d.tolist() == [[32, 12, 50, 30, np.float32(.9)], [40, 20, 77, 47, np.float32(.7)]]  # translated by (30, 10)


def test_a_box_over_a_frame_side_edge_is_clipped_and_translated():
    d, src = _fold1([[-5, -3, 20, 20, .9], [-5, -3, 47.25, 20, .8]], CORNER0)
    assert src.tolist() == [0] and d[:, :4].tolist() == [[0, 0, 20, 20]]
    # the bottom-right tile: clipped to ITS last pixel (49, 39), which is the frame's (99, 59)
    d, src = _fold1([[30, 25, 60, 45, .9], [1.75, 25, 60, 45, .8], [30, 25, 1000, 45, .7]], CORNER1)
    assert src.tolist() == [0, 2] and d[:, :4].tolist() == [[80, 45, 99, 59], [80, 45, 99, 59]]
    # past an INTERIOR side the same box goes: it runs into the holder's padding, or the neighbour's pixels
    assert _fold1([[30, 25, 60, 30, .9]], MIDDLE)[1].tolist() == []
    assert _fold1([[-1, 25, 20, 30, .9]], MIDDLE)[1].tolist() == []
    # the seam rule reads the UNCLIPPED box: clipped first, [30, 25, 49, 30] would have passed a limit of 49
    assert _fold1([[30, 25, 60, 30, .9]], [30, 10, 50, 40, 2, 2, 49, 39])[1].tolist() == []


def test_rows_beyond_the_tile_go():
    rows = [[49, 5, 60, 10, .9],      # x1 == tw - 1: touches the last column
            [49.25, 5, 60, 10, .8],   # beyond it
            [5, 39, 10, 50, .7],      # y1 == th - 1
            [5, 40, 10, 50, .6],
            [-10, -10, 0, 0, .5],     # x2 == 0 and y2 == 0: touches the first pixel
            [-10, -10, -0.25, 5, .4],
            [5, -10, 10, -1, .3]]
    d, src = _fold1(rows, [10, 5, 50, 40, -INF, -INF, INF, INF])
    assert src.tolist() == [0, 2, 4]
    assert d[:, :4].tolist() == [[59, 10, 59, 15], [15, 44, 20, 44], [10, 5, 10, 5]]


def test_nan_rows_are_dropped():
    nan = np.nan
    rows = [[5, 5, 9, 9, .9], [nan, 5, 9, 9, .8], [5, nan, 9, 9, .7], [6, 6, 9, 9, .6], [5, 5, nan, 9, .5], [5, 5, 9, nan, .4]]
    for tile in (MIDDLE, CORNER0, [0, 0, 100, 60, -INF, -INF, INF, INF]):
        for flip in (0, 1):
            assert _fold1(rows, tile, flip=flip)[1].tolist() == [0, 3]
    d, src = _fold1([[5, 5, 9, 9, nan]], MIDDLE)  # a NaN score is not a coordinate
    assert src.tolist() == [0] and np.isnan(d[0, 4])


def test_area_window_is_of_the_clipped_translated_box():
    rows = [[2, 2, 11, 11, .9], [2, 2, 11, 12, .8], [2, 2, 12, 12, .7], [2, 2, 5, 5, .6]]  # areas 100, 110, 121, 16
    assert _fold1(rows, MIDDLE, lo=100, hi=121)[1].tolist() == [0, 1]
    assert _fold1(rows, MIDDLE, lo=-INF, hi=100)[1].tolist() == [3]
    # 20 x 20 hanging over the tile's (and the frame's) corner leaves 10 x 10
    assert _fold1([[40, 30, 59, 49, .5]], CORNER1, lo=100, hi=101)[1].tolist() == [0]


def test_a_mirrored_tile_is_translated_in_the_mirrored_frame_and_then_unmirrored():
    # the tile at (50, 20) of the MIRRORED 100-wide frame covers columns 0 .. 49 of the real one
    d, src = _fold1([[10, 5, 20, 15, .9], [30, 25, 60, 45, .8]], CORNER1, flip=1)
    assert src.tolist() == [0, 1]
    assert d[:, :4].tolist() == [[99 - 70, 25, 99 - 60, 35], [99 - 99, 45, 99 - 80, 59]]
    # the seam is the mirrored tile's: its LEFT side is interior
    assert _fold1([[1.75, 5, 20, 15, .9]], CORNER1, flip=1)[1].tolist() == []


def test_layout_and_argument_errors_of_the_restatement():
    B, V, C = 2, 3, 2
    lists = [np.asarray([[p, p, p + 1, p + 1, .5]] * (p + 1), np.float32) for p in range(B * V * C)]
    table = np.asarray([FRAME + [0, -INF, INF, 7, 3, 50, 40, -INF, -INF, INF, INF]] * (B * V), np.float32)
    r = PP.fold_tiles_numpy(lists, table, V, C)
    assert r["source"].tolist() == [0, 2, 4, 1, 3, 5, 6, 8, 10, 7, 9, 11]  # q = (i * C + c) * V + v
    for q, p in enumerate(r["source"]):
        assert r["dets"][q][:, :4].tolist() == [[p + 7, p + 3, p + 8, p + 4]] * (p + 1)
    with pytest.raises(ValueError, match="fold_tiles_numpy"):
        PP.fold_tiles_numpy(lists[:5], table, V, C)
    with pytest.raises(ValueError, match="fold_tiles_numpy"):
        PP.fold_tiles_numpy(lists, table[:, :12], V, C)


def test_a_whole_frame_tile_row_is_the_view_fold():
    """zero offsets, (tw, th) = (fw, fh), infinite limits: on the view suite's own inputs the tile fold keeps the rows the
    view fold keeps. Equal as VALUES: a -0 comes back +0 from the translation."""
    for name, (B, V, Cn) in VC.FOLD_SHAPES.items():
        lists, table = VC.fold_inputs(name)[:2]
        t13 = np.concatenate((table[:, :5], np.tile(np.asarray([[0, 0, VC.FW, VC.FH, -INF, -INF, INF, INF]], np.float32),
                                                    (len(table), 1))), 1)
        ref, got = VC.fold_reference(name), PP.fold_tiles_numpy(lists, t13, V, Cn)
        assert got["counts"].tolist() == ref["counts"].tolist() and got["source"].tolist() == ref["source"].tolist()
        for q in range(len(lists)):
            assert got["src_row"][q].tolist() == ref["src_row"][q].tolist()
            assert np.array_equal(got["dets"][q], ref["dets"][q])


# ---- the cases of the GPU file ------------------------------------------------------------------------------------------

def test_fold_cases_cover_what_they_claim():
    lengths, seen = set(), set()
    for name, (B, V, C) in TC.FOLD_SHAPES.items():
        lists, table, packed, counts, offsets, reasons = TC.fold_inputs(name)
        spec = TC._fold_spec(name)[0]
        assert len(lists) == B * V * C and table.shape == (B * V, TC.STRIDE) and np.all(table[:, 13:] == TC.MARKER)
        lengths |= set(int(c) for c in counts)
        ref = TC.fold_reference(name)
        for q, p in enumerate(ref["source"]):
            # the pattern the rows were built from is what the restatement keeps, and for the reason they were built with
            stays = [k for k, why in enumerate(reasons[p]) if why in ("inside", "on_limit", "clipped")]
            assert ref["src_row"][q].tolist() == stays, (name, p, spec[p])
            seen |= set(reasons[p])
        # multiples of a quarter pixel below 2^11: translation and mirroring are exact
        fin = packed[:, :4][np.isfinite(packed[:, :4])]
        assert np.all(fin * 4 == np.round(fin * 4)) and np.abs(fin).max() < 2 ** 11
        t = table[:, 5:13][np.isfinite(table[:, 5:13])]
        assert np.all(t * 4 == np.round(t * 4))
        assert all(int(offsets[p + 1]) > int(offsets[p]) + int(counts[p]) for p in range(len(lists) - 1))
    assert seen == set(TC.REASONS), set(TC.REASONS) - seen
    assert lengths >= {0, 1, 63, 64, 65, 255, 256, 257, 1000}
    assert TC.fold_reference("b1v1c1")["src_row"][0].tolist() == [0]
    last = TC.fold_reference("b1v2c1")
    assert last["src_row"][0].tolist() == [255] and last["src_row"][1].tolist() == [255, 511, 767]
    ref = TC.fold_reference("b2v5c2")
    n_in = [int(TC.fold_inputs("b2v5c2")[3][p]) for p in ref["source"]]
    pats = dict(none=False, all=False, other=False)
    for q in range(len(n_in)):
        if n_in[q] >= 2:
            pats["none"] |= int(ref["counts"][q]) == n_in[q]
            pats["all"] |= int(ref["counts"][q]) == 0
            pats["other"] |= ref["src_row"][q].tolist() == list(range(0, n_in[q], 2))
    assert all(pats.values()), pats
    # a kept row of a translated tile moved, a clipped one changed, a mirrored one was mirrored
    lists, table = TC.fold_inputs("b1v10c3")[:2]
    ref = TC.fold_reference("b1v10c3")
    assert any(len(ref["dets"][q]) and not np.array_equal(ref["dets"][q][:, 1], lists[p][ref["src_row"][q]][:, 1])
               for q, p in enumerate(ref["source"]))


def test_margins_of_the_chained_gpu_cases():
    """what makes test_gpu_tiles.py's chained comparisons meaningful: on the FOLDED lists of every case it runs, the float64
    merge's suppression margin and -- under gaussian or with voting -- the restatement's pick and drop margins hold; the fold
    lands on the clusters again; the seam rule removes the clusters a tile's side cuts, and only from that tile"""
    import soft_merge_cases as C
    checked = 0
    for name in TC.CHAINED:
        lists, table, B, V, Cn = TC.chained_inputs(name)
        folded = TC.folded_reference(name)
        n_in = sum(len(q) for q in lists)
        assert 0 < int(folded["counts"].sum()) < n_in  # the seams cut some clusters
        clean = TC.chained_clean(name)
        for q, p in enumerate(folded["source"]):
            kept = clean[p][folded["src_row"][q]]
            assert np.abs(folded["dets"][q][:, :4] - kept[:, :4]).max(initial=0) <= 2e-3
            if np.isinf(table[p // Cn, 9:13]).all():  # the full-frame view loses nothing
                assert len(kept) == len(clean[p])
        assert any(table[iv, 2] for iv in range(B * V)) and any(table[iv, 5] > 0 for iv in range(B * V))
        hard = PP.merge_numpy(folded["dets"], V, C.THR)
        assert hard["margin"] >= C.MARGIN, (name, hard["margin"])
        assert int(hard["counts"].sum()) < int(folded["counts"].sum())  # the tiles overlap: the merge suppresses
        for method, vote in TC.CHAINED_RUNS:
            ref = TC.chained_reference(name, method, vote)
            if C.needs_margin(method, vote):
                m = ref["margin"]
                assert m["pick"] >= C.MARGIN and m["drop"] >= C.MARGIN, (name, method, vote, m)
                L = max(int(folded["counts"][l * V:(l + 1) * V].sum()) for l in range(B * Cn))
                assert method != "gaussian" or L <= 80, (name, L)
            assert set(np.concatenate(ref["group"]).tolist()) == set(range(V)), (name, method, vote)  # every view contributes
            checked += 1
    assert checked == len(TC.CHAINED) * 6


# ---- the C entry point without a GPU ------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_tile_fold():
    protos = _lib.parse_header()
    assert "dana_detect_fold_tiles" in protos and hasattr(ctypes.CDLL(_lib.LIB_PATH), "dana_detect_fold_tiles")
    args = lambda n: [(t, a) for t, a in protos[n][1]]  # noqa: E731
    assert args("dana_detect_fold_tiles") == args("dana_detect_fold_views")  # the view fold's signature
    assert _lib.lib().query("dana_abi_version") == 1  # the change is additive


def test_tile_fold_argument_errors_are_reported_without_a_gpu():
    L = _lib.lib()
    p, o = 16, 32  # (never dereferenced: every call below returns before its launch)
    call = lambda *a: L.call("dana_detect_fold_tiles", *a)  # noqa: E731
    for k in (0, 1, 2, 6, 8, 9, 10):  # every pointer but src_row_out, which may be null
        a = [p, p, p, 1, 2, 3, p, 13, o, p, p, None, None]
        a[k] = None
        with pytest.raises(_lib.DanaError, match="dana_detect_fold_tiles: null pointer"):
            call(*a)
    with pytest.raises(_lib.DanaError, match="dana_detect_fold_tiles: view_stride 12 < 13"):
        call(p, p, p, 1, 2, 3, p, 12, o, p, p, p, None)
    with pytest.raises(_lib.DanaError, match="dana_detect_fold_tiles: dets_out must not alias dets_in"):
        call(p, p, p, 1, 2, 3, p, 13, p, p, p, p, None)
    with pytest.raises(_lib.DanaError, match="bad shape"):
        call(p, p, p, 1, -2, 3, p, 13, o, p, p, p, None)
    with pytest.raises(_lib.DanaError, match="lists"):
        call(p, p, p, 1 << 20, 1 << 10, 4, p, 13, o, p, p, p, None)
    for shape in ((0, 2, 3), (1, 0, 3), (1, 2, 0)):  # zero size: DANA_OK before anything is looked at
        call(None, None, None, *shape, None, 0, None, None, None, None, None)


def test_python_argument_errors_come_before_any_c_call():
    class _CD(list):
        packed = counts = offsets = layout_dev = None
        num_classes = 2
    z = np.zeros(6)
    tiles = PL.TileSet(2, 3, np.zeros((6, 13), np.float32), np.ones(6), z, np.zeros((6, 4)))
    with pytest.raises(ValueError, match="fold_tiles: 5 images in the detections, but 2 images x 3 views"):
        PP.fold_tiles(_CD([[]] * 5), tiles)
    with pytest.raises(ValueError, match="5 images in the detections"):  # ensemble_views folds a TileSet with fold_tiles
        PP.ensemble_views(_CD([[]] * 5), tiles)
    with pytest.raises(ValueError, match="fold_tiles: needs the TileSet"):
        PP.fold_tiles(_CD([[]] * 6), PL.ViewSet(2, 3, np.zeros((6, 5), np.float32), np.ones(6), z))
    with pytest.raises(ValueError, match="fold them with fold_tiles"):
        PP.fold_views(_CD([[]] * 6), tiles)
    with pytest.raises(ValueError, match="method"):
        PP.ensemble_views(None, tiles, method="soft")
