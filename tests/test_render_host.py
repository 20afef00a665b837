"""Host suite of dana_amd.render: the numpy restatements of the three kernels (boxes_numpy, sheet_numpy, to_rgb_numpy)
against hand-worked pixels, the label text and font, the sheet geometry, the PNG / PPM writers and the argument errors.
The GPU suite (test_gpu_render.py) then demands bit equality of the device results with these restatements."""
import numpy as np
import pytest
import torch

from dana_amd import render as R
from dana_amd.config import cfg
from oracle.pipeline_ref import cv_resize_linear
from render_cases import decode_png

WHITE = np.array([[255, 255, 255]], np.uint8)


def one_list(n):
    """the counts | offsets layout of a single list of n rows"""
    return np.array([n, 0, n], np.int32)


def draw(boxes, h=12, w=16, **kw):
    boxes = np.asarray(boxes, np.float32).reshape(-1, 5)
    kw.setdefault("colors", WHITE)
    kw.setdefault("layout", one_list(len(boxes)))
    return R.boxes_numpy(np.zeros((1, h, w, 3), np.uint8), boxes, **kw)[0]


def extent(img):
    ys, xs = np.nonzero(img.any(-1))
    return int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())


# box, thickness, scale, pixels, (row_lo, row_hi, col_lo, col_hi) or None: worked by hand on a 12 x 16 canvas
HAND = [
    ((3.7, 2.2, 9.9, 8.0), 1, 1.0, 24, (2, 8, 3, 9)),
    ((3.7, 2.2, 9.9, 8.0), 2, 1.0, 56, (1, 9, 2, 10)),
    ((3.7, 2.2, 9.9, 8.0), 3, 1.0, 72, (1, 9, 2, 10)),
    ((-5, -5, 4, 4), 2, 1.0, 20, None),
    ((5, 5, 5, 5), 1, 1.0, 1, None),
    ((5, 5, 6, 6), 2, 1.0, 16, None),
    ((1.5, 1.5, 4.9, 3.9), 2, 2.0, 48, (2, 8, 2, 10)),
]


@pytest.mark.parametrize("box,t,scale,pixels,ext", HAND)
def test_hand_worked_boxes(box, t, scale, pixels, ext):
    img = draw([list(box) + [0.5]], thickness=t, scale=scale)
    assert int(img.any(-1).sum()) == pixels
    if ext is not None:
        assert extent(img) == ext
    assert set(np.unique(img)) <= {0, 255}


def test_band_pixels_of_thickness_one():
    img = draw([[3.7, 2.2, 9.9, 8.0, 1.0]]).any(-1)
    want = np.zeros((12, 16), bool)
    want[2, 3:10] = want[8, 3:10] = want[2:9, 3] = want[2:9, 9] = True
    assert np.array_equal(img, want)


def test_painting_order():
    pal = np.array([[10, 20, 30], [200, 100, 50]], np.uint8)
    boxes = [[2, 2, 8, 8, 0.9], [5, 5, 12, 10, 0.8]]
    idx = np.array([0, 1], np.int32)
    first = draw(boxes, colors=pal, color_index=idx, top="first")
    last = draw(boxes, colors=pal, color_index=idx, top="last")
    # (8, 5) and (5, 8) lie on both outlines
    assert tuple(first[8, 5]) == (10, 20, 30) and tuple(first[5, 8]) == (10, 20, 30)
    assert tuple(last[8, 5]) == (200, 100, 50) and tuple(last[5, 8]) == (200, 100, 50)
    assert np.array_equal(first.any(-1), last.any(-1))
    # a pixel only one box covers has that box's colour either way
    assert tuple(first[2, 2]) == tuple(last[2, 2]) == (10, 20, 30)
    assert tuple(first[10, 12]) == tuple(last[10, 12]) == (200, 100, 50)


def test_class_slot_colours_wrap():
    pal = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    boxes = np.array([[1, 1, 3, 3, .5], [5, 1, 7, 3, .5], [9, 1, 11, 3, .5]], np.float32)
    layout = np.array([1, 1, 1, 0, 1, 2, 3], np.int32)  # one image, three class slots
    img = R.boxes_numpy(np.zeros((1, 12, 16, 3), np.uint8), boxes, layout=layout, lists_per_image=3, colors=pal)[0]
    assert tuple(img[1, 1]) == (1, 2, 3) and tuple(img[1, 5]) == (4, 5, 6) and tuple(img[1, 9]) == (1, 2, 3)


def test_tile_and_chunk_constants():
    """the sizes the device suite builds its canvases and row counts around"""
    assert R.TILE == (16, 64) and R.LIST_CHUNK == 256


def test_color_index_shorter_than_the_buffer():
    """a color_index covers the rows it has; a row at or beyond its end takes its class slot (a MergedDetections' packed
    buffer is longer than its `group`)"""
    pal = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    boxes = [[1, 1, 3, 3, .5], [5, 1, 7, 3, .5], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    img = draw(boxes, colors=pal, color_index=np.array([1], np.int32), layout=one_list(2))
    assert tuple(img[1, 1]) == (4, 5, 6) and tuple(img[1, 5]) == (1, 2, 3)
    img = draw(boxes, colors=pal, color_index=np.array([-1, 3, 0, 0, 0, 0], np.int32), layout=one_list(2))  # modulo 2
    assert tuple(img[1, 1]) == (4, 5, 6) and tuple(img[1, 5]) == (4, 5, 6)


def test_empty_batch_and_canvas_bounds():
    out = R.boxes_numpy(np.zeros((0, 4, 4, 3), np.uint8), np.zeros((1, 5), np.float32), layout=np.zeros(1, np.int32))
    assert out.shape == (0, 4, 4, 3)
    with pytest.raises(ValueError, match="empty batch"):
        R.boxes_numpy(np.zeros((0, 4, 4, 3), np.uint8), np.zeros((1, 5), np.float32), layout=one_list(1))
    # the C entry point refuses a canvas taller than its grid can cover as an argument error, before any launch
    from dana_amd._lib import DanaError, lib
    tall = (1, 65535 * R.TILE[0] + 1, 8)
    with pytest.raises(DanaError, match="bad canvas"):
        lib().call("dana_render_draw_boxes", 8, *tall, 8, 5, 0, 8, 8, 1, None, 0, None, 1.0, 1, 0, 0.0, 8, 1, None, 0, None, 0,
                   0, None)


def test_skip_rules():
    nan, inf = float("nan"), float("inf")
    for bad in ([nan, 2, 8, 8, .5], [2, 2, inf, 8, .5], [2, -inf, 8, 8, .5], [2, 2, 8, 8, nan], [8, 2, 2, 8, .5],
                [2, 8, 8, 2, .5]):
        assert not draw([bad]).any(), bad
    # truncation decides "inverted": (5.9, 5.2) -> (5, 5) is a point, (6.0, 5.9) is inverted
    assert draw([[5.9, 5.9, 5.2, 5.2, .5]]).any(-1).sum() == 1
    assert not draw([[6.0, 5, 5.9, 5, .5]]).any()
    # huge finite coordinates are clamped, not skipped: the outline of (-1e30, 4) .. (1e30, 6) crosses the canvas twice
    img = draw([[-1e30, 4, 1e30, 6, .5]]).any(-1)
    assert img[4].all() and img[6].all() and img.sum() == 32
    # min_score: >= keeps
    assert draw([[2, 2, 8, 8, 0.5]], min_score=0.5).any()
    assert not draw([[2, 2, 8, 8, 0.5]], min_score=0.5000001).any()
    # a zero scale collapses every box onto pixel (0, 0); an Inf product is skipped
    assert draw([[2, 2, 8, 8, 0.5]], scale=0.0).any(-1).sum() == 1
    assert not draw([[2, 2, 8, 8, 0.5]], scale=1e38).any()


def test_ground_truth_form():
    gt = np.zeros((2, 4, 5), np.float32)
    gt[0, 0] = [1, 1, 4, 4, 3]
    gt[0, 1] = [6, 1, 9, 4, 0]     # class 0: not drawn (fsod_logger.py:76)
    gt[0, 2] = [11, 1, 14, 4, 2]   # beyond num_boxes[0] = 2
    gt[1, 0] = [1, 6, 4, 9, 1]
    img = R.boxes_numpy(np.zeros((2, 12, 16, 3), np.uint8), gt.reshape(-1, 5), per_image=4, num_boxes=np.array([2, 1]),
                        colors=WHITE).any(-1)
    assert img[0, 1, 1] and not img[0, 1, 6] and not img[0, 1, 11] and img[0].sum() == 12
    assert img[1, 6, 1] and img[1].sum() == 12
    # num_boxes larger than the holder reads K rows, not the next image's
    img = R.boxes_numpy(np.zeros((2, 12, 16, 3), np.uint8), gt.reshape(-1, 5), per_image=4, num_boxes=np.array([9, 0]),
                        colors=WHITE).any(-1)
    assert img[0, 1, 11] and img[0].sum() == 24 and not img[1].any()


def test_layout_rows_outside_the_buffer_draw_nothing():
    boxes = np.array([[2, 2, 8, 8, .5]], np.float32)
    for layout in ([1, 5, 6], [1, -1, 0], [-3, 0, 0]):
        assert not R.boxes_numpy(np.zeros((1, 12, 16, 3), np.uint8), boxes, layout=np.array(layout, np.int32)).any()


def test_font():
    assert len(R.FONT) == len(R.CHARS) == 12 and R.CHARS == "0123456789. "
    for glyph in R.FONT:
        assert len(glyph) == 7 and all(len(row) == 5 and set(row) <= {"#", "."} for row in glyph)
    assert len(set(R.FONT)) == 12
    rows = np.asarray(R.FONT_ROWS)
    assert rows.shape == (12, 7) and rows.max() < 32
    assert rows[1, 0] == 0b00100 and rows[2, 6] == 0b11111 and not rows[11].any()
    assert all(np.asarray(R.FONT_ROWS[k]).any() for k in range(11))


def test_label_text():
    assert R.label_text(0.875, 12) == "12 0.88"
    assert R.label_text(1.0, 3) == "3 1.00" and R.label_text(1.0, 3).endswith(" 1.00")
    assert R.label_text(0.0, 0) == "0 0.00" and R.label_text(-2.0, 0) == "0 0.00" and R.label_text(7.5, 0) == "0 1.00"
    assert R.label_text(0.004999, 1) == "1 0.00" and R.label_text(0.005, 1) == "1 0.01"
    assert R.label_text(17.0) == "17" and R.label_text(3.9) == "3" and R.label_text(-1.0) == "0"
    assert R.label_text(1e9) == "9999" and R.label_text(0.5, 123456) == "9999 0.50"
    assert set(R.label_text(0.123, 4567) + R.label_text(89.0)) <= set(R.CHARS)


def test_label_geometry():
    green = np.array([[0, 204, 0]], np.uint8)       # luma 119: white glyphs
    yellow = np.array([[255, 255, 0]], np.uint8)    # luma 226: black glyphs
    # room above: "0 0.50" is 6 characters -> the bar is 37 x 9 at (X1 - h, Y1 - h - 9) = (4, 10)
    img = draw([[5, 20, 60, 35, 0.5]], h=40, w=70, labels=True, thickness=2, colors=green)
    bar = img[10:19, 4:41]
    assert (bar.reshape(-1, 3) == green[0]).all(1).sum() + (bar.reshape(-1, 3) == 255).all(1).sum() == 37 * 9
    assert not img[9, 4:41].any() and not img[10:19, 41].any() and not img[10:19, 3].any()
    assert (bar[0] == green[0]).all() and (bar[8] == green[0]).all() and (bar[:, 0] == green[0]).all()
    # the first glyph is FONT[0], one pixel in from the bar's corner
    glyph = np.array([[c == "#" for c in row] for row in R.FONT[0]])
    assert np.array_equal((bar[1:8, 1:6] == 255).all(-1), glyph)
    # ... and the '.' (4th character) sits in cell 3
    dot = np.array([[c == "#" for c in row] for row in R.FONT[10]])
    assert np.array_equal((bar[1:8, 19:24] == 255).all(-1), dot)
    # a light colour takes black glyphs
    img_y = draw([[5, 20, 60, 35, 0.5]], h=40, w=70, labels=True, thickness=2, colors=yellow)
    assert np.array_equal((img_y[11:18, 5:10] == 0).all(-1), glyph)
    # no room above (Y1 - h - 9 < 0): the bar flips inside, to (X1 - h, Y1 + g) = (4, 6), over the left band
    img = draw([[5, 5, 60, 35, 0.5]], h=40, w=70, labels=True, thickness=2, colors=green)
    assert np.array_equal((img[7:14, 5:10] == 255).all(-1), glyph)
    assert not img[:4].any() and (img[4:6, 4:62] == green[0]).all()
    assert (img[6:15, 4:41].reshape(-1, 3) != 0).any(1).all() and not img[6:15, 41:60].any()
    # Y1 - h - 9 == 0 still fits above
    img = draw([[5, 10, 60, 35, 0.5]], h=40, w=70, labels=True, thickness=2, colors=green)
    assert np.array_equal((img[1:8, 5:10] == 255).all(-1), glyph) and (img[0, 4:41] == green[0]).all()
    # clipped at the right edge: a canvas 20 wide keeps the bar's first 16 columns
    img = draw([[5, 20, 60, 35, 0.5]], h=40, w=20, labels=True, thickness=2, colors=green)
    assert img.shape == (40, 20, 3) and (img[10, 4:20] == green[0]).all()
    assert np.array_equal((img[11:18, 5:10] == 255).all(-1), glyph)
    # the ground-truth form prints the class alone: "7" -> a bar 7 wide
    gt = np.array([[5, 20, 60, 35, 7.0]], np.float32)
    img = R.boxes_numpy(np.zeros((1, 40, 70, 3), np.uint8), gt, per_image=1, num_boxes=np.array([1]), labels=True,
                        colors=green)[0]
    assert img[11:20, 5:12].any(-1).all() and not img[11:20, 12].any() and not img[10, 5:12].any()


def test_to_rgb_numpy():
    means = np.asarray(cfg.PIXEL_MEANS, np.float32).reshape(-1)  # (B, G, R)
    im = np.zeros((3, 1, 5), np.float32)
    for c in range(3):
        im[c, 0] = np.array([10.5, -3.0, 300.0, np.nan, 254.5], np.float32) - means[c]
    im[:, 0, 3] = np.nan
    out = R.to_rgb_numpy(im)
    assert out.shape == (1, 5, 3) and out.dtype == np.uint8
    assert out[0, 1].tolist() == [0, 0, 0] and out[0, 2].tolist() == [255, 255, 255] and out[0, 3].tolist() == [0, 0, 0]
    # the channel order flips: plane 0 (B) lands in out[..., 2]
    im2 = -np.broadcast_to(means[:, None, None], (3, 2, 2)).astype(np.float32).copy()
    im2[0] += 7
    im2[2] += 200
    assert R.to_rgb_numpy(im2)[0, 0].tolist() == [200, 0, 7]
    # halves round up, as (unsigned char)(v + 0.5) does
    exact = np.zeros((3, 1, 2), np.float32)
    exact[:, 0, 0], exact[:, 0, 1] = 10.5, 10.49
    assert R.to_rgb_numpy(exact, means_bgr=(0, 0, 0))[0].tolist() == [[11, 11, 11], [10, 10, 10]]


@pytest.mark.parametrize("S,cols", [(1, 1), (3, 2), (5, 3)])
def test_sheet_geometry(S, cols):
    H, W, side, pad = 40, 30, 16, 4
    rpc, ncol, out_w, corners = R.sheet_geometry(H, W, S, side, pad)
    assert rpc == 2 and ncol == cols and out_w == W + cols * 20
    assert corners == [(34 + (s // 2) * 20, (s % 2) * 20) for s in range(S)]
    rng = np.random.RandomState(S)
    q = rng.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    sup = rng.randint(0, 200, (2, S, 16, 16, 3)).astype(np.uint8)  # side x side shots: the resize is the identity
    out = R.sheet_numpy(q, sup, side, pad, pad_value=255)
    assert out.shape == (2, H, out_w, 3) and np.array_equal(out[:, :, :W], q)
    covered = np.zeros((H, out_w), bool)
    covered[:, :W] = True
    for s, (x, y) in enumerate(corners):
        assert np.array_equal(out[:, y:y + side, x:x + side], sup[:, s])
        covered[y:y + side, x:x + side] = True
    assert (out[:, ~covered] == 255).all()
    assert (R.sheet_numpy(q, sup, side, pad, pad_value=7)[:, ~covered] == 7).all()


def test_sheet_single_column_and_tall_shots():
    # side + pad > H - side: one row per column, one column per shot
    rpc, cols, out_w, corners = R.sheet_geometry(20, 10, 3, 16, 4)
    assert (rpc, cols, out_w) == (1, 3, 70) and corners == [(14, 0), (34, 0), (54, 0)]
    assert R.sheet_geometry(16, 10, 2, 16, 0)[:3] == (1, 2, 42)
    assert R.sheet_geometry(600, 1000, 3)[:3] == (3, 1, 1164)


@pytest.mark.parametrize("hs,ws,side", [(20, 20, 7), (7, 7, 20), (9, 14, 16), (16, 16, 16), (1, 1, 5)])
def test_resize_agrees_with_cv_resize(hs, ws, side):
    shot = np.random.RandomState(hs * 100 + ws).randint(0, 256, (hs, ws, 3)).astype(np.uint8)
    ref = cv_resize_linear(shot.astype(np.float32), dsize=(side, side))
    ref = (np.clip(ref, 0, 255) + np.float32(0.5)).astype(np.uint8)
    got = R.resize_numpy(shot, side)
    assert got.shape == (side, side, 3)
    assert np.abs(got.astype(np.int32) - ref.astype(np.int32)).max() <= 1
    if hs == ws == side:
        assert np.array_equal(got, shot)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_write_png(tmp_path, as_tensor):
    rgb = np.random.RandomState(3).randint(0, 256, (5, 7, 3)).astype(np.uint8)
    path = str(tmp_path / "a.png")
    R.write_png(path, torch.from_numpy(rgb) if as_tensor else rgb)
    assert np.array_equal(decode_png(open(path, "rb").read()), rgb)
    # a non-contiguous view is written as it reads
    R.write_png(path, rgb[:, ::2])
    assert np.array_equal(decode_png(open(path, "rb").read()), rgb[:, ::2])


def test_write_ppm(tmp_path):
    rgb = np.random.RandomState(4).randint(0, 256, (3, 9, 3)).astype(np.uint8)
    path = str(tmp_path / "a.ppm")
    R.write_ppm(path, torch.from_numpy(rgb))
    data = open(path, "rb").read()
    head = b"P6\n9 3\n255\n"
    assert data[:len(head)] == head
    assert np.array_equal(np.frombuffer(data[len(head):], np.uint8).reshape(3, 9, 3), rgb)


def test_value_errors(tmp_path):
    cpu_img = torch.zeros(1, 3, 4, 4)
    with pytest.raises(ValueError, match="CUDA"):
        R.to_rgb(cpu_img)
    with pytest.raises(ValueError):
        R.to_rgb(cpu_img.double())
    canvas = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA"):
        R.draw_boxes(canvas, torch.zeros(1, 5), torch.tensor([1, 0, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="CUDA"):
        R.sheet(canvas, torch.zeros(1, 1, 4, 4, 3, dtype=torch.uint8), side=4)
    z = np.zeros((2, 12, 16, 3), np.uint8)
    b = np.zeros((4, 5), np.float32)
    lay = np.array([2, 2, 0, 2, 4], np.int32)
    for kw in (dict(layout=lay, top="middle"), dict(layout=lay, thickness=0), dict(layout=lay, thickness=1.5),
               dict(layout=lay, thickness=R.MAX_THICKNESS + 1), dict(), dict(per_image=2), dict(num_boxes=np.array([1, 1])),
               dict(layout=lay, per_image=2, num_boxes=np.array([1, 1])), dict(layout=lay[:4]),
               dict(layout=lay, lists_per_image=2), dict(layout=np.array([1, 1, 1, 0, 1, 2, 3], np.int32)),
               dict(per_image=3, num_boxes=np.array([1, 1])), dict(per_image=2, num_boxes=np.array([1])),
               dict(layout=lay, scale=np.ones(3, np.float32)), dict(layout=lay, color_index=np.zeros((2, 2), np.int32)),
               dict(layout=lay, colors=np.zeros((0, 3), np.uint8))):
        with pytest.raises(ValueError):
            R.boxes_numpy(z, b, **kw)
    with pytest.raises(ValueError):
        R.boxes_numpy(z, b[:, :4], layout=lay)
    with pytest.raises(ValueError):
        R.boxes_numpy(z[0], b, layout=lay)
    q, sup = np.zeros((1, 20, 10, 3), np.uint8), np.zeros((1, 2, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="side"):
        R.sheet_numpy(q, sup, side=21)
    for kw in (dict(side=0), dict(pad=-1), dict(pad_value=256)):
        with pytest.raises(ValueError):
            R.sheet_numpy(q, sup, **dict(dict(side=8), **kw))
    with pytest.raises(ValueError):
        R.sheet_numpy(q, sup[0], side=8)
    with pytest.raises(ValueError):
        R.sheet_numpy(np.zeros((2, 20, 10, 3), np.uint8), sup, side=8)
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            R.write_png(str(tmp_path / "x.png"), bad)
        with pytest.raises(ValueError):
            R.write_ppm(str(tmp_path / "x.ppm"), bad)
    with pytest.raises(ValueError):
        R.prediction_sheet(cpu_img, torch.zeros(1, 3), object(), torch.zeros(1, 1, 3, 4, 4))
