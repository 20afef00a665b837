"""dana_amd.render on the device (csrc/render.hip): every result must equal the module's numpy restatement BYTE FOR BYTE
(np.array_equal) -- the kernels and the restatements apply the same integer rule to the same fp32 products, and the
sheet's interpolation runs the same fp32 operations in the same order (no fused multiply-add on either side).

Shapes. The rasteriser's tile is render.TILE = 16 rows x 64 columns and its LDS list holds render.LIST_CHUNK = 256
boxes; an image's list counts are scanned 256 lists at a time. Canvases: 1 x 1, 5 x 7, 37 x 53 (three partial tiles
down), 32 x 128 (exactly 2 x 2 tiles) and 33 x 129 (one pixel more each way: 3 x 3 tiles); N = 3 images of 0, 1 and 300
rows (300 > LIST_CHUNK: a second chunk of rows, and on the one-tile canvases a second fill of the list); 300 lists per
image (> 256: a second scan)."""
import os

import numpy as np
import pytest
import torch

from render_cases import decode_png, random_boxes

pytestmark = pytest.mark.gpu

CANVASES = [(1, 1), (5, 7), (37, 53), (32, 128), (33, 129)]
ROWS = (0, 1, 300)
PAL2 = np.array([[250, 240, 10], [20, 30, 200]], np.uint8)  # one light colour (black glyphs), one dark (white glyphs)


def _layout(counts, offsets=None):
    counts = np.asarray(counts, np.int32)
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    return np.concatenate((counts, offsets)).astype(np.int32)


def _dev(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def both(dev, canvas, boxes, **kw):
    """draw on the device and with the restatement -> (device result as numpy, restatement)"""
    from dana_amd import render as R
    ref = R.boxes_numpy(canvas, boxes, **kw)
    dkw = dict(kw)
    for name in ("layout", "num_boxes", "colors", "color_index"):
        if dkw.get(name) is not None:
            dkw[name] = _dev(np.asarray(dkw[name]), dev)
    if isinstance(dkw.get("scale"), np.ndarray):
        dkw["scale"] = _dev(dkw["scale"], dev)
    c = _dev(canvas, dev)
    out = R.draw_boxes(c, _dev(boxes, dev), **dkw)
    assert out is c
    return out.cpu().numpy(), ref


def test_to_rgb(dev):
    from dana_amd import attention, render as R
    from dana_amd.config import cfg
    means = np.asarray(cfg.PIXEL_MEANS, np.float32).reshape(-1)
    rng = np.random.RandomState(0)
    im = np.zeros((2, 3, 5, 7), np.float32)
    k = rng.randint(0, 255, im.shape).astype(np.float32)
    for c in range(3):
        im[:, c] = k[:, c] + np.float32(0.5) - means[c]   # at the rounding boundary
    im[0, :, 0, 0] = -400.0
    im[0, :, 0, 1] = 400.0
    im[0, 1, 0, 2] = np.nan
    im[1, :, 4, 6] = np.nan
    im[1, 0, 2, 3] = np.inf
    im[1, 2, 2, 4] = -np.inf
    out = R.to_rgb(_dev(im, dev))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 5, 7, 3)
    got = out.cpu().numpy()
    assert np.array_equal(got, R.to_rgb_numpy(im))
    assert got[0, 0, 0].tolist() == [0, 0, 0] and got[0, 0, 1].tolist() == [255, 255, 255] and got[0, 0, 2, 1] == 0
    assert got[1, 4, 6].tolist() == [0, 0, 0] and got[1, 2, 3, 2] == 255 and got[1, 2, 4, 0] == 0
    # leading dimensions are kept, and a square input equals the attention overlay at alpha = 0 bit for bit
    sq = (rng.randn(2, 3, 3, 9, 9) * 90).astype(np.float32)
    sq[0, 0, :, 0, 0] = np.nan
    sq[1, 2, 1] = np.round(sq[1, 2, 1]) + np.float32(0.5) - means[1]
    d_sq = _dev(sq, dev)
    rgb = R.to_rgb(d_sq)
    assert tuple(rgb.shape) == (2, 3, 9, 9, 3) and np.array_equal(rgb.cpu().numpy(), R.to_rgb_numpy(sq))
    maps = _dev(rng.rand(2, 3, 4, 5).astype(np.float32), dev)
    assert torch.equal(attention.render(maps, d_sq, alpha=0), rgb)


CONFIGS = [  # thickness, labels, top
    (1, False, "first"), (2, True, "first"), (3, False, "last"), (8, True, "last"), (50, False, "first"), (1, True, "last"),
    (64, True, "first"),
]


@pytest.mark.parametrize("H,W", CANVASES)
def test_draw_boxes_canvases(dev, H, W):
    """N = 3 images of 0, 1 and 300 seeded random rows (every kind of render_cases.KINDS), one class slot, over a random
    background: each thickness (50 and 64 exceed most boxes), labels on and off, both painting orders"""
    rng = np.random.RandomState(H * 1000 + W)
    canvas = rng.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    boxes = random_boxes(rng, sum(ROWS), H, W)
    assert np.isnan(boxes).any() and np.isinf(boxes).any() and (np.abs(boxes[np.isfinite(boxes)]) >= 1e30).any()
    layout = _layout(ROWS)
    for t, labels, top in CONFIGS:
        got, ref = both(dev, canvas, boxes, layout=layout, thickness=t, labels=labels, top=top, colors=PAL2)
        assert np.array_equal(got, ref), (t, labels, top, int((got != ref).any(-1).sum()))
        assert np.array_equal(got[0], canvas[0])  # the image without rows
        assert (got[2] != canvas[2]).any()
    # what no box covers keeps the random background: 20 rows of image 2 alone leave most of a larger canvas alone
    few = _layout((0, 1, 20))
    got, ref = both(dev, canvas, boxes, layout=few, thickness=1, colors=PAL2)
    untouched = (ref == canvas).all(-1)
    assert np.array_equal(got, ref) and np.array_equal(got[untouched], canvas[untouched])
    if H * W > 64:
        assert untouched[2].any() and (~untouched[2]).any()


def test_every_kind_of_row(dev):
    """each kind alone on a 37 x 53 canvas, thickness 2 with labels: the rows that must draw nothing draw nothing"""
    from render_cases import KINDS
    H, W = 37, 53
    for kind in KINDS:
        rng = np.random.RandomState(len(kind))
        boxes = random_boxes(rng, 6, H, W, kinds=(kind,))
        canvas = rng.randint(0, 256, (1, H, W, 3)).astype(np.uint8)
        got, ref = both(dev, canvas, boxes, layout=_layout([6]), thickness=2, labels=True, colors=PAL2)
        assert np.array_equal(got, ref), kind
        assert (got != canvas).any() == (kind not in ("outside", "inverted", "nan", "inf")), kind


@pytest.mark.parametrize("top", ["first", "last"])
def test_list_refill_keeps_painting_order(dev, top):
    """300 boxes of 2 x 1 pixels, each sharing a pixel with the next row's, on ONE tile, a colour per row: 300 survivors
    > LIST_CHUNK, so the list is painted, emptied and filled again; the pixels settled by the first
    fill must survive the second, and every row keeps a pixel of its own under either painting order"""
    from dana_amd import render as R
    n = 300
    i = np.arange(n)
    x, y = i % 63, i // 63 * 3 + 1
    boxes = np.stack([x, y, x + 1, y, np.full(n, 0.5)], 1).astype(np.float32)
    pal = np.stack([i % 251 + 1, i // 2 + 1, 255 - i % 200], 1).astype(np.uint8)
    assert len({tuple(p) for p in pal}) == n
    canvas = np.zeros((1, R.TILE[0], R.TILE[1], 3), np.uint8)
    got, ref = both(dev, canvas, boxes, layout=_layout([n]), thickness=1, colors=pal, color_index=i.astype(np.int32), top=top)
    assert np.array_equal(got, ref)
    assert {tuple(p) for p in got.reshape(-1, 3)} == {tuple(p) for p in pal} | {(0, 0, 0)}
    # where rows 10 and 11 overlap, the painting order decides
    assert tuple(got[0, 1, 11]) == tuple(pal[10 if top == "first" else 11])


@pytest.mark.parametrize("L", [1, 3])
def test_class_slots_palette_scale_and_color_index(dev, L):
    """N = 2 images x L class slots with uneven lists (one empty, offsets not in list order), a palette of 2 colours that
    wraps over 3 slots, a different scale per image, min_score; then the same with a color_index tensor"""
    H, W, N = 37, 53, 2
    rng = np.random.RandomState(10 + L)
    counts = np.array([5, 0, 7, 2, 40, 1][:N * L] if L == 3 else [9, 46], np.int32)
    total = int(counts.sum())
    boxes = np.concatenate((random_boxes(rng, total, H // 2, W // 2), np.zeros((3, 5), np.float32)))  # 3 rows no list owns
    order = rng.permutation(N * L)  # list p's rows start where the lists before it IN THIS ORDER end
    offsets = np.zeros(N * L + 1, np.int32)
    pos = 0
    for p in order:
        offsets[p] = pos
        pos += counts[p]
    offsets[N * L] = total
    layout = _layout(counts, offsets)
    canvas = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    scale = np.array([2.0, 0.75], np.float32)
    for kw in (dict(), dict(min_score=0.5), dict(color_index=rng.randint(-3, 9, len(boxes)).astype(np.int32), top="last")):
        got, ref = both(dev, canvas, boxes, layout=layout, lists_per_image=L, scale=scale, thickness=2, labels=True,
                        colors=PAL2, **kw)
        assert np.array_equal(got, ref), kw
        assert (got[0] != canvas[0]).any() and (got[1] != canvas[1]).any()
    # a Python-number scale and the default palette
    got, ref = both(dev, canvas, boxes, layout=layout, lists_per_image=L, scale=1.5, thickness=3, labels=True)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("top", ["first", "last"])
def test_more_lists_than_one_scan(dev, top):
    """300 lists per image (> 256: the counts are scanned in two batches), 0 to 2 rows each, N = 2; labels print slots
    of one to three digits"""
    H, W, N, L = 33, 129, 2, 300
    rng = np.random.RandomState(77)
    counts = rng.randint(0, 3, N * L).astype(np.int32)
    boxes = random_boxes(rng, int(counts.sum()), H, W, kinds=("inside", "point", "left", "bottom"))
    canvas = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    got, ref = both(dev, canvas, boxes, layout=_layout(counts), lists_per_image=L, thickness=1, labels=True, colors=PAL2, top=top)
    assert np.array_equal(got, ref)


def _merged(dev, H, W):
    """2 images x 3 lists of jittered boxes around shared objects, merged per image with NMS: rows are suppressed, so the
    packed buffer is longer than `total` and `group` is shorter than it"""
    from dana_amd import postprocess as PP
    rng = np.random.RandomState(31)
    counts = np.array([6, 4, 5, 3, 0, 7], np.int32)
    total = int(counts.sum())
    ctr = rng.uniform([8, 8], [W - 8, H - 8], size=(4, 2))
    o = rng.randint(0, 4, total)
    cxy = ctr[o] + rng.normal(0, 1.0, size=(total, 2))
    wh = rng.uniform(8, 14, size=(4, 2))[o]
    score = ((rng.permutation(total) + 1.0) / (total + 1.0))[:, None]
    rows = np.concatenate((cxy - wh / 2, cxy + wh / 2, score), 1).astype(np.float32)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    for p in range(6):  # each list in descending score order, as NMS output is
        seg = rows[offsets[p]:offsets[p + 1]]
        rows[offsets[p]:offsets[p + 1]] = seg[np.argsort(-seg[:, 4], kind="stable")]
    packed = torch.from_numpy(rows).to(dev)
    cd = PP.ClassDetections([[packed[offsets[b * 3 + c]:offsets[b * 3 + c + 1]] for c in range(3)] for b in range(2)])
    cd.packed, cd.counts, cd.offsets, cd.num_classes = packed, torch.from_numpy(counts), torch.from_numpy(offsets), 3
    cd.layout_dev = torch.from_numpy(np.concatenate((counts, offsets))).to(dev)
    return PP.merge_detections(cd, 3, nms_thresh=0.3, with_layout=True), total


def test_merged_detections_coloured_by_group(dev):
    """a `merge_detections(..., with_layout=True)` result drawn with color_index = its `group`: `packed` has more rows
    than `group` has entries (NMS removed some), which draw_boxes and prediction_sheet must take as they are"""
    from dana_amd import render as R
    H, W = 37, 53
    m, n_in = _merged(dev, H, W)
    assert 0 < m.total < n_in and m.group.numel() == m.total < m.packed.size(0)
    assert len(set(m.group.cpu().tolist())) > 1
    rng = np.random.RandomState(32)
    canvas = rng.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    pal = np.array([[250, 240, 10], [20, 30, 200], [200, 20, 20]], np.uint8)
    packed, layout, group = m.packed.cpu().numpy(), m.layout_dev.cpu().numpy(), m.group.cpu().numpy()
    ref = R.boxes_numpy(canvas, packed, layout=layout, thickness=2, labels=True, colors=pal, color_index=group)
    got = R.draw_boxes(_dev(canvas, dev), m.packed, m.layout_dev, thickness=2, labels=True, colors=_dev(pal, dev),
                       color_index=m.group)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert all((ref == pal[g]).all(-1).any() for g in set(group.tolist()))  # every group's colour is on the canvas
    # a row at or beyond the end of color_index takes its class slot
    short = group[:2]
    got, ref = both(dev, canvas, packed, layout=layout, thickness=2, colors=pal, color_index=short)
    assert np.array_equal(got, ref)
    # ... and the same through prediction_sheet, which takes the MergedDetections itself
    im = torch.from_numpy((rng.randn(2, 3, H, W) * 64).astype(np.float32)).to(dev)
    sup = torch.from_numpy((rng.randn(2, 2, 3, 12, 12) * 64).astype(np.float32)).to(dev)
    info = torch.tensor([[H, W, 1.0], [H, W, 0.5]], dtype=torch.float32, device=dev)
    sheet = R.prediction_sheet(im, info, m, sup, thickness=1, colors=_dev(pal, dev), color_index=m.group, side=16, pad=2)
    drawn = R.boxes_numpy(R.to_rgb_numpy(im.cpu().numpy()), packed, layout=layout, scale=np.array([1.0, 0.5], np.float32),
                          thickness=1, labels=True, colors=pal, color_index=group)
    assert np.array_equal(sheet.cpu().numpy(), R.sheet_numpy(drawn, R.to_rgb_numpy(sup.cpu().numpy()), side=16, pad=2))


def test_empty_batch(dev):
    from dana_amd import render as R
    canvas = torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=dev)
    out = R.draw_boxes(canvas, torch.zeros((1, 5), device=dev), torch.zeros(1, dtype=torch.int32, device=dev), labels=True)
    assert out is canvas and tuple(out.shape) == (0, 8, 8, 3)


def test_ground_truth_form(dev):
    """gt_boxes [N, K, 5].view(-1, 5) with num_boxes < K (int32 and int64), class-0 rows, a num_boxes above K"""
    H, W, N, K = 37, 53, 3, 6
    rng = np.random.RandomState(5)
    gt = random_boxes(rng, N * K, H, W, kinds=("inside", "left", "point")).reshape(N, K, 5)
    gt[:, :, 4] = rng.randint(0, 25, (N, K))
    gt[0, 1, 4] = 0
    gt[1, 0, 4] = 12345
    canvas = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    for nb in ([4, 0, 2], [6, 9, 1]):
        for dtype in (np.int32, np.int64):
            got, ref = both(dev, canvas, gt.reshape(-1, 5), per_image=K, num_boxes=np.asarray(nb, dtype), thickness=2,
                            labels=True, colors=PAL2)
            assert np.array_equal(got, ref), (nb, dtype)
    assert np.array_equal(got[0], ref[0]) and (got[1] != canvas[1]).any()


def test_two_runs_give_the_same_bytes(dev):
    from dana_amd import render as R
    H, W = 37, 53
    rng = np.random.RandomState(8)
    canvas = rng.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    boxes, layout = _dev(random_boxes(rng, sum(ROWS), H, W), dev), _dev(_layout(ROWS), dev)
    runs = [R.draw_boxes(_dev(canvas, dev), boxes, layout, thickness=3, labels=True) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])


def test_device_argument_errors(dev):
    from dana_amd import render as R
    canvas = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=dev)
    boxes = torch.zeros((4, 5), device=dev)
    layout = _dev(_layout([2, 2]), dev)
    for kw in (dict(layout=layout.cpu()), dict(layout=layout.long()), dict(layout=layout, thickness=0),
               dict(layout=layout, top="up"), dict(), dict(per_image=2), dict(layout=layout, lists_per_image=2),
               dict(layout=layout, scale=torch.ones(3, device=dev)), dict(layout=layout, scale=torch.ones(2)),
               dict(layout=layout, colors=torch.zeros((2, 3), device=dev)), dict(layout=layout, color_index=torch.zeros((2, 2), dtype=torch.int32, device=dev)),
               dict(layout=layout, color_index=torch.zeros(4, dtype=torch.int64, device=dev)),
               dict(per_image=3, num_boxes=torch.ones(2, dtype=torch.int32, device=dev)),
               dict(per_image=2, num_boxes=torch.ones(2, dtype=torch.int32))):
        with pytest.raises(ValueError):
            R.draw_boxes(canvas, boxes, **kw)
    with pytest.raises(ValueError):
        R.draw_boxes(canvas.float(), boxes, layout)
    with pytest.raises(ValueError):
        R.draw_boxes(canvas, boxes[:, :4].contiguous(), layout)
    q = torch.zeros((1, 20, 10, 3), dtype=torch.uint8, device=dev)
    sup = torch.zeros((1, 2, 8, 8, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="side"):
        R.sheet(q, sup, side=21)
    with pytest.raises(ValueError):
        R.sheet(q, sup.float(), side=8)
    with pytest.raises(ValueError):
        R.to_rgb(torch.zeros((2, 4, 5, 5), device=dev))
    assert not canvas.any()


@pytest.mark.parametrize("S", [1, 3, 5])
@pytest.mark.parametrize("hs,ws", [(20, 20), (7, 7), (9, 14)])
def test_sheet(dev, S, hs, ws):
    """H = 40, side = 16, pad = 4: two rows per column, 1 / 2 / 3 columns; 20 -> 16 shrinks, 7 -> 16 grows, 9 x 14 is not
    square. Then 20 -> 7 and 7 -> 20 proper in a single-column sheet (H = 20)."""
    from dana_amd import render as R
    rng = np.random.RandomState(S * 100 + hs)
    q = rng.randint(0, 256, (2, 40, 30, 3)).astype(np.uint8)
    sup = rng.randint(0, 256, (2, S, hs, ws, 3)).astype(np.uint8)
    out = R.sheet(_dev(q, dev), _dev(sup, dev), side=16, pad=4, pad_value=200)
    ref = R.sheet_numpy(q, sup, side=16, pad=4, pad_value=200)
    assert tuple(out.shape) == (2, 40, 30 + 20 * ((S + 1) // 2), 3) and np.array_equal(out.cpu().numpy(), ref)
    side = 7 if hs == 20 else 20
    q1 = q[:, :side + 2]
    out = R.sheet(_dev(q1, dev), _dev(sup, dev), side=side, pad=3)
    ref = R.sheet_numpy(q1, sup, side=side, pad=3)
    assert R.sheet_geometry(side + 2, 30, S, side, 3)[0] == 1 and tuple(out.shape) == (2, side + 2, 30 + S * (side + 3), 3)
    assert np.array_equal(out.cpu().numpy(), ref)


def test_sheet_without_shots_and_without_pad(dev):
    from dana_amd import render as R
    rng = np.random.RandomState(2)
    q = rng.randint(0, 256, (1, 16, 5, 3)).astype(np.uint8)
    out = R.sheet(_dev(q, dev), torch.zeros((1, 0, 4, 4, 3), dtype=torch.uint8, device=dev), side=8)
    assert np.array_equal(out.cpu().numpy(), q)
    sup = rng.randint(0, 256, (1, 3, 4, 6, 3)).astype(np.uint8)
    out = R.sheet(_dev(q, dev), _dev(sup, dev), side=8, pad=0, pad_value=0)
    assert tuple(out.shape) == (1, 16, 5 + 16, 3) and np.array_equal(out.cpu().numpy(), R.sheet_numpy(q, sup, 8, 0, 0))


def test_replayed_without_reading_anything_back(dev):
    """draw_boxes with a layout and labels, recorded into a LaunchProgram (which refuses any device-to-host read): one
    C-ABI launch and no torch op. Boxes, layout, scale and canvas are then overwritten IN PLACE with a second case of other
    counts, and the replay must draw that case."""
    from dana_amd import program, render as R
    H, W, N, L = 37, 53, 2, 2
    rng = np.random.RandomState(21)
    cases = []
    for counts in ([3, 1, 0, 4], [0, 2, 5, 1]):
        boxes = np.zeros((8, 5), np.float32)
        boxes[:sum(counts)] = random_boxes(rng, sum(counts), H, W, kinds=("inside", "left", "point", "top"))
        cases.append(dict(canvas=rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8), boxes=boxes, layout=_layout(counts),
                          scale=rng.uniform(0.5, 1.5, N).astype(np.float32)))
    first, second = cases
    canvas, boxes, layout, scale = (_dev(first[k], dev) for k in ("canvas", "boxes", "layout", "scale"))
    colors = _dev(PAL2, dev)
    kw = dict(lists_per_image=L, thickness=2, labels=True, colors=colors)
    R.draw_boxes(canvas.clone(), boxes, layout, scale=scale, **kw)  # (the font is on the device from here on)
    p = program.LaunchProgram(dev)
    with p.recording():
        R.draw_boxes(canvas, boxes, layout, scale=scale, **kw)
    assert p.stats["launches"] == 1 and p.stats["torch_ops"] == 0
    ref = R.boxes_numpy(first["canvas"], first["boxes"], layout=first["layout"], scale=first["scale"], lists_per_image=L,
                        thickness=2, labels=True, colors=PAL2)
    assert np.array_equal(canvas.cpu().numpy(), ref)
    for t, k in ((canvas, "canvas"), (boxes, "boxes"), (layout, "layout"), (scale, "scale")):
        t.copy_(torch.from_numpy(second[k]))
    p.run()
    torch.cuda.synchronize()
    ref = R.boxes_numpy(second["canvas"], second["boxes"], layout=second["layout"], scale=second["scale"], lists_per_image=L,
                        thickness=2, labels=True, colors=PAL2)
    assert not np.array_equal(ref, second["canvas"]) and np.array_equal(canvas.cpu().numpy(), ref)


def test_prediction_and_episode_sheets_end_to_end(dev, tmp_path):
    """a tiny episode through the eval forward and detections_by_class(with_layout=True): the prediction sheet equals the
    composition of the three restatements on the same device outputs, and the PNG written from it decodes to it"""
    import dana_amd
    from dana_amd import postprocess, render as R, synthetic as Sy
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=2, classes=["fg", "bg"])
    m.load_state_dict(Sy.fill_state_dict(m.state_dict(), seed=5, profile="test"))
    m.to(dev).eval()
    im, info, gt, nb, sup = [t.to(dev) for t in Sy.episode_inputs(1, 1, 2, 128, 160, seed=9)]
    info = info.clone()
    info[:, 2] = 0.8  # (detections are divided by the scale; drawing multiplies them back)
    with torch.no_grad():
        out = m(im, info, gt, nb, sup)
    dets = postprocess.detections_by_class(out[0], out[1], out[2], info, 1, with_layout=True)
    assert int(dets.counts.sum()) > 0
    sheet = R.prediction_sheet(im, info, dets, sup, thickness=2, side=48, pad=4)
    canvas = R.boxes_numpy(R.to_rgb_numpy(im.cpu().numpy()), dets.packed.cpu().numpy(), layout=dets.layout_dev.cpu().numpy(),
                           scale=info[:, 2].cpu().numpy(), thickness=2, labels=True)
    ref = R.sheet_numpy(canvas, R.to_rgb_numpy(sup.cpu().numpy()), side=48, pad=4)
    got = sheet.cpu().numpy()
    assert got.shape == (1, 128, 160 + 52, 3) and np.array_equal(got, ref)
    assert (canvas != R.to_rgb_numpy(im.cpu().numpy())).any()  # something was drawn
    # the (packed, layout_dev) pair is the same call
    assert torch.equal(R.prediction_sheet(im, info, (dets.packed, dets.layout_dev), sup, thickness=2, side=48, pad=4), sheet)
    path = os.path.join(str(tmp_path), "prediction.png")
    R.write_png(path, sheet[0])
    assert np.array_equal(decode_png(open(path, "rb").read()), got[0])
    # the training episode's figure: ground truth on the query, the first shot beside it (one way: no negative shot)
    ep = R.episode_sheet(im, gt, nb, sup, shot=2, side=48)
    canvas = R.boxes_numpy(R.to_rgb_numpy(im.cpu().numpy()), gt.cpu().numpy().reshape(-1, 5), per_image=gt.size(1),
                           num_boxes=nb.cpu().numpy(), thickness=2, labels=True)
    ref = R.sheet_numpy(canvas, R.to_rgb_numpy(sup[:, :1].cpu().numpy()), side=48)
    assert np.array_equal(ep.cpu().numpy(), ref)
