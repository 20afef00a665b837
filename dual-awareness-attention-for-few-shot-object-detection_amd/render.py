"""The prediction figure on the device: a query image with its boxes and labels drawn, the support shots beside it
(the reference's README images/prediction.jpg, FSODLogger._add_images / FSODInferenceLogger, net_utils.vis_detections,
utils.plot_box), from what is already resident there: the prepared images, the packed detection buffer with its
`layout_dev`, gt_boxes / num_boxes, the evaluator's marks. Nothing here reads device memory back to the host except the
two writers at the end (`write_png`, `write_ppm`).

    to_rgb            prepared images (BGR planes minus cfg.PIXEL_MEANS) -> RGB bytes          dana_render_to_rgb
    draw_boxes        outlines and labels of every box of every image, in place, one launch     dana_render_draw_boxes
    sheet             the query | its support shots, resized and laid out in columns            dana_render_sheet
    prediction_sheet  the three composed for detections; episode_sheet for a training episode

The pixel rule of `draw_boxes` is this project's own (cv2's thick-line and text rasterisers are not restated: nothing here
could pin them). A row (x1, y1, x2, y2, v) drawn with thickness t into image b:
  1. every coordinate is multiplied by scale[b] in fp32; a row whose product is NaN or Inf, or whose v is NaN, is skipped;
     X1 = (int)clamp(x1 * scale, -2^20, 2^20) (truncation toward zero), X2, Y1, Y2 likewise;
  2. a row with X2 < X1 or Y2 < Y1 is skipped;
  3. h = t // 2, g = t - h;
  4. the band is the outer rectangle [X1-h, X2+h] x [Y1-h, Y2+h] minus the inner one [X1+g, X2-g] x [Y1+g, Y2-g],
     inside the canvas (an empty inner rectangle leaves the band filled);
  5. with labels on, a bar 6 * nchars + 1 wide and 9 high in the box's colour, its top-left corner at (X1-h, Y1-h-9), or
     at (X1-h, Y1+g) -- just inside the top band -- when Y1-h-9 < 0; the text in FONT's 5x7 glyphs, 6x8 cells, starting
     one pixel in from the bar's top-left, black when the colour's (299 R + 587 G + 114 B) // 1000 >= 128 and white
     otherwise. The bar is clipped to the canvas and lies over its own box's band;
  6. a pixel takes the colour of the topmost box whose band or bar covers it; a pixel nothing covers is not written.
`boxes_numpy`, `to_rgb_numpy` and `sheet_numpy` restate the three kernels in numpy (host): the tests' yardsticks, equal
to the device results bit for bit."""
import struct
import zlib

import numpy as np
import torch

from . import ops
from .config import cfg

CHARS = "0123456789. "
# 5x7 glyphs of CHARS, drawn for this project ('#' set); a label cell is 6x8: one empty column right, one empty row below
FONT = (
    (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),  # 0
    ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),  # 1
    (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),  # 2
    (".###.", "#...#", "....#", "..##.", "....#", "#...#", ".###."),  # 3
    ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),  # 4
    ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),  # 5
    (".###.", "#....", "#....", "####.", "#...#", "#...#", ".###."),  # 6
    ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),  # 7
    (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),  # 8
    (".###.", "#...#", "#...#", ".####", "....#", "....#", ".###."),  # 9
    (".....", ".....", ".....", ".....", ".....", ".##..", ".##.."),  # .
    (".....", ".....", ".....", ".....", ".....", ".....", "....."),  # space
)
# what the kernel reads: [12][7] bytes, bit 4 the glyph's left column
FONT_ROWS = tuple(tuple(sum(1 << (4 - x) for x in range(5) if row[x] == "#") for row in glyph) for glyph in FONT)

# box colours by class slot (R, G, B); the first is vis_detections' green (net_utils.py:58)
DEFAULT_COLORS = ((0, 204, 0), (255, 64, 64), (64, 128, 255), (255, 200, 0), (255, 0, 255), (0, 220, 220), (255, 128, 0),
                  (160, 96, 255))

TILE = (16, 64)    # rows x columns of canvas one workgroup of dana_render_draw_boxes rasterises
LIST_CHUNK = 256   # boxes its LDS list holds: an image with more boxes on one tile is painted in several fills
MAX_THICKNESS = 1024
MAX_LABEL_NUMBER = 9999  # the largest class slot / ground-truth class a label prints (larger values print as this)
_COORD = np.float32(1 << 20)

_CONST = {}  # (device, what) -> uint8 device tensor of FONT_ROWS / DEFAULT_COLORS


def _means():
    return [float(v) for v in torch.as_tensor(cfg.PIXEL_MEANS).reshape(-1).tolist()]  # (B, G, R)


def _device_const(dev, what, rows):
    key = (str(dev), what)
    t = _CONST.get(key)
    if t is None:
        t = _CONST[key] = torch.tensor(rows, dtype=torch.uint8).to(dev)
    return t


def _cuda(t, name, dtype, who):
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise ValueError("%s: %s must be a %s tensor, got %s" % (who, name, dtype, t.dtype if torch.is_tensor(t) else type(t)))
    if not t.is_cuda:
        raise ValueError("%s: %s must be a CUDA (HIP) tensor: this build has no CPU path" % (who, name))
    return t


# ---- to_rgb ----------------------------------------------------------------------------------------------------------------

def to_rgb(images):
    """float32 [..., 3, H, W] prepared images (BGR, mean-subtracted, as the model is fed) -> uint8 [..., H, W, 3] RGB:
    out[y][x][c] = clamp(round(image[2-c][y][x] + PIXEL_MEANS[2-c]), 0, 255), NaN -> 0. The rounding is
    `attention.render`'s, so render(maps, images, alpha=0) equals to_rgb(images) bit for bit. One launch."""
    _cuda(images, "images", torch.float32, "to_rgb")
    if images.dim() < 3 or images.size(-3) != 3:
        raise ValueError("to_rgb: images must be float32 [..., 3, H, W], got %s" % (tuple(images.shape),))
    return ops.render_to_rgb(images.contiguous(), _means())


def to_rgb_numpy(images, means_bgr=None):
    """`to_rgb` restated in numpy float32 (host)"""
    im = np.asarray(images, np.float32)
    means = np.asarray(_means() if means_bgr is None else means_bgr, np.float32)
    rgb = np.moveaxis(im[..., ::-1, :, :], -3, -1) + means[::-1]
    return (np.fmin(np.fmax(rgb, np.float32(0)), np.float32(255)) + np.float32(0.5)).astype(np.uint8)


# ---- draw_boxes ------------------------------------------------------------------------------------------------------------

def label_text(v, slot=None):
    """the label of a row: "<slot> <s.ss>" with hundredths (int)(v * 100 + 0.5) clamped to 0..100 (fp32), or for the
    ground-truth form (slot None) "<v as integer>"; numbers above MAX_LABEL_NUMBER print as MAX_LABEL_NUMBER"""
    v = np.float32(v)
    if slot is None:
        return "%d" % int(min(max(v, np.float32(0)), np.float32(MAX_LABEL_NUMBER)))
    hund = int(min(max(v * np.float32(100) + np.float32(0.5), np.float32(0)), np.float32(100)))
    return "%d %d.%02d" % (min(int(slot), MAX_LABEL_NUMBER), hund // 100, hund % 100)


def _check_draw(who, layout_len, N, lists_per_image, per_image, has_num_boxes, thickness, top):
    """the host-side argument rules shared by draw_boxes and boxes_numpy -> (lists per image, top_last)"""
    if top not in ("first", "last"):
        raise ValueError('%s: top must be "first" or "last", got %r' % (who, top))
    if int(thickness) != thickness or not 1 <= int(thickness) <= MAX_THICKNESS:
        raise ValueError("%s: thickness must be an integer in 1..%d, got %r" % (who, MAX_THICKNESS, thickness))
    if layout_len is not None:
        if per_image is not None or has_num_boxes:
            raise ValueError("%s: give either layout or per_image with num_boxes, not both" % who)
        n = (layout_len - 1) // 2
        if layout_len != 2 * n + 1:
            raise ValueError("%s: layout must hold counts [n] | offsets [n+1] (2n+1 values), got %d" % (who, layout_len))
        if lists_per_image is None and N == 0:
            if n:
                raise ValueError("%s: a layout of %d lists for an empty batch of images" % (who, n))
            return 1, top == "last"  # (no images, no lists: nothing to draw, as the C entry point takes it)
        L = n // N if lists_per_image is None else lists_per_image
        if int(L) < 1 or int(L) > MAX_LABEL_NUMBER + 1 or int(L) * N != n:
            raise ValueError("%s: %d lists do not split into %d images x lists_per_image = %s" % (who, n, N, L))
        return int(L), top == "last"
    if per_image is None or not has_num_boxes:
        raise ValueError("%s: without a layout give per_image=K and num_boxes [N] (the ground-truth form)" % who)
    if lists_per_image not in (None, 1):
        raise ValueError("%s: lists_per_image belongs to the layout form" % who)
    if int(per_image) < 0:
        raise ValueError("%s: per_image must be >= 0, got %s" % (who, per_image))
    return 1, top == "last"


def draw_boxes(canvas, boxes, layout=None, lists_per_image=None, per_image=None, num_boxes=None, scale=1.0, thickness=1,
               min_score=None, colors=None, color_index=None, labels=False, top="first"):
    """Draw the outlines (labels=True: and labels) of `boxes` into `canvas`, uint8 [N, H, W, 3] on the device, in place;
    returns the canvas. One launch however many boxes there are; no argument is read on the host.

    boxes: float32 [M, >=5] rows (x1, y1, x2, y2, v), either
      * a packed detection buffer (v the score) with `layout`, the int32 counts | offsets tensor [2n+1] of
        `ClassDetections.layout_dev` for n = N * lists_per_image lists (default: n // N): list p belongs to image
        p // lists_per_image and has class slot p % lists_per_image; or
      * gt_boxes.view(-1, 5) (v the class) with per_image=K and num_boxes int32 (or int64) [N]: rows at or beyond
        num_boxes[b] and rows with v == 0 are not drawn (fsod_logger.py:76).
    scale: float32 [N] device tensor or a number; detections are in original-image pixels and the canvas is the prepared
    image: pass im_info[:, 2]. min_score: rows with v < min_score are skipped. colors: uint8 [P, 3] device palette
    (default DEFAULT_COLORS), indexed by class slot modulo P (the ground-truth form has one slot, 0: every box and label
    in colors[0]) or by color_index modulo P: a one-dimensional int32 device tensor with one entry per packed row, such
    as `MergedDetections.group`, whose `total` entries cover every row its layout reaches (`packed` is longer); a row
    at or beyond its end takes its class slot. An evaluator's `tpfp` marks are uint8 [T, n] by RANK: scatter one
    threshold's row through `EvalResult.order` into an int32 [n] tensor by detection row first. top: which end of an image's row order is painted on
    top; NMS output is score-descending, so "first" puts the best box on top. The pixel rule: module docstring."""
    who = "draw_boxes"
    _cuda(canvas, "canvas", torch.uint8, who)
    if canvas.dim() != 4 or canvas.size(3) != 3 or not canvas.is_contiguous():
        raise ValueError("draw_boxes: canvas must be a contiguous uint8 [N, H, W, 3] tensor, got %s" % (tuple(canvas.shape),))
    _cuda(boxes, "boxes", torch.float32, who)
    if boxes.dim() != 2 or boxes.size(1) < 5 or not boxes.is_contiguous():
        raise ValueError("draw_boxes: boxes must be contiguous float32 [M, >=5] rows (x1, y1, x2, y2, v), got %s"
                         % (tuple(boxes.shape),))
    N = canvas.size(0)
    if layout is not None:
        _cuda(layout, "layout", torch.int32, who)
        if layout.dim() != 1 or not layout.is_contiguous():
            raise ValueError("draw_boxes: layout must be a contiguous int32 [2n+1] tensor, got %s" % (tuple(layout.shape),))
    L, top_last = _check_draw(who, None if layout is None else layout.numel(), N, lists_per_image, per_image,
                              num_boxes is not None, thickness, top)
    counts_ptr = offsets_ptr = None
    if layout is not None:
        counts_ptr, offsets_ptr = layout.data_ptr(), layout.data_ptr() + 4 * (N * L)
    else:
        if not torch.is_tensor(num_boxes) or num_boxes.dtype not in (torch.int32, torch.int64):
            raise ValueError("draw_boxes: num_boxes must be an int32 (or int64) [N] tensor")
        if not num_boxes.is_cuda:
            raise ValueError("draw_boxes: num_boxes must be a CUDA (HIP) tensor: this build has no CPU path")
        num_boxes = num_boxes.reshape(-1).to(torch.int32).contiguous()
        if num_boxes.numel() != N or N * int(per_image) > boxes.size(0):
            raise ValueError("draw_boxes: %d images x per_image = %d need num_boxes [%d] and at least %d rows, got %d and %d"
                             % (N, per_image, N, N * int(per_image), num_boxes.numel(), boxes.size(0)))
    if torch.is_tensor(scale):
        _cuda(scale, "scale", torch.float32, who)
        scale = scale.reshape(-1).contiguous()
        if scale.numel() != N:
            raise ValueError("draw_boxes: scale must hold one value per image (%d), got %d" % (N, scale.numel()))
    if colors is None:
        colors = _device_const(canvas.device, "colors", DEFAULT_COLORS)
    _cuda(colors, "colors", torch.uint8, who)
    if colors.dim() != 2 or colors.size(1) != 3 or colors.size(0) < 1 or not colors.is_contiguous():
        raise ValueError("draw_boxes: colors must be a contiguous uint8 [P >= 1, 3] palette, got %s" % (tuple(colors.shape),))
    if color_index is not None:
        _cuda(color_index, "color_index", torch.int32, who)
        if color_index.dim() != 1 or not color_index.is_contiguous():
            raise ValueError("draw_boxes: color_index must be a contiguous one-dimensional int32 tensor, got %s"
                             % (tuple(color_index.shape),))
    font = _device_const(canvas.device, "font", FONT_ROWS) if labels else None
    return ops.render_draw_boxes(canvas, boxes, counts_ptr, offsets_ptr, L, num_boxes, 0 if per_image is None else int(per_image),
                                 scale, int(thickness), min_score, colors, color_index, font, bool(labels), top_last)


def _trunc(v):
    return int(min(max(v, -_COORD), _COORD))


def boxes_numpy(canvas, boxes, layout=None, lists_per_image=None, per_image=None, num_boxes=None, scale=1.0, thickness=1,
                min_score=None, colors=None, color_index=None, labels=False, top="first"):
    """`draw_boxes` restated in numpy (host), on arrays of the same shapes and meanings; returns a drawn COPY of `canvas`.
    Boxes are painted from the bottom of the painting order to its top, each over what is there."""
    who = "boxes_numpy"
    out = np.array(canvas, dtype=np.uint8)
    if out.ndim != 4 or out.shape[3] != 3:
        raise ValueError("boxes_numpy: canvas must be uint8 [N, H, W, 3], got %s" % (out.shape,))
    boxes = np.asarray(boxes, np.float32)
    if boxes.ndim != 2 or boxes.shape[1] < 5:
        raise ValueError("boxes_numpy: boxes must be float32 [M, >=5] rows (x1, y1, x2, y2, v), got %s" % (boxes.shape,))
    N, H, W = out.shape[:3]
    M = boxes.shape[0]
    if layout is not None:
        layout = np.asarray(layout, np.int64).reshape(-1)
    L, top_last = _check_draw(who, None if layout is None else layout.size, N, lists_per_image, per_image,
                              num_boxes is not None, thickness, top)
    t = int(thickness)
    h = t // 2
    g = t - h
    pal = np.asarray(DEFAULT_COLORS if colors is None else colors, np.uint8).reshape(-1, 3)
    if pal.shape[0] < 1:
        raise ValueError("boxes_numpy: colors must be a uint8 [P >= 1, 3] palette")
    scale_b = np.broadcast_to(np.asarray(scale, np.float32).reshape(-1), (N,)) if np.size(scale) in (1, N) else None
    if scale_b is None:
        raise ValueError("boxes_numpy: scale must hold one value per image (%d), got %d" % (N, np.size(scale)))
    if color_index is not None:
        color_index = np.asarray(color_index, np.int64)
        if color_index.ndim != 1:
            raise ValueError("boxes_numpy: color_index must be one-dimensional, got %s" % (color_index.shape,))
    if layout is None:
        num_boxes = np.asarray(num_boxes, np.int64).reshape(-1)
        if num_boxes.size != N or N * int(per_image) > M:
            raise ValueError("boxes_numpy: %d images x per_image = %d need num_boxes [%d] and at least %d rows"
                             % (N, per_image, N, N * int(per_image)))
    glyphs = (np.asarray(FONT_ROWS, np.uint8)[:, :, None] >> np.arange(4, -1, -1) & 1).astype(bool)  # [12][7][5]
    for b in range(N):
        order = []  # (row, slot) in the image's row order
        for s in range(L):
            if layout is not None:
                cnt, off = int(layout[b * L + s]), int(layout[N * L + b * L + s])
            else:
                cnt, off = min(int(num_boxes[b]), int(per_image)), b * int(per_image)
            order += [(off + i, s) for i in range(min(max(cnt, 0), M))]
        img = out[b]
        for r, slot in (order if top_last else reversed(order)):
            if not 0 <= r < M:
                continue
            sc = scale_b[b]
            with np.errstate(over="ignore", invalid="ignore"):
                prod = [boxes[r, j] * sc for j in range(4)]
            v = boxes[r, 4]
            if not all(np.isfinite(p) for p in prod) or np.isnan(v):
                continue
            if layout is None and v == 0:
                continue
            if min_score is not None and v < np.float32(min_score):
                continue
            X1, Y1, X2, Y2 = (_trunc(p) for p in prod)
            if X2 < X1 or Y2 < Y1:
                continue
            ci = int(color_index[r]) if color_index is not None and r < color_index.size else slot
            col = pal[ci % pal.shape[0]]
            # the band
            ox0, ox1, oy0, oy1 = max(X1 - h, 0), min(X2 + h, W - 1), max(Y1 - h, 0), min(Y2 + h, H - 1)
            if ox0 <= ox1 and oy0 <= oy1:
                ys = np.arange(oy0, oy1 + 1)[:, None]
                xs = np.arange(ox0, ox1 + 1)[None, :]
                inner = (xs >= X1 + g) & (xs <= X2 - g) & (ys >= Y1 + g) & (ys <= Y2 - g)
                img[oy0:oy1 + 1, ox0:ox1 + 1][~inner] = col
            if not labels:
                continue
            text = label_text(v, None if layout is None else slot)
            bx, by = X1 - h, (Y1 - h - 9 if Y1 - h - 9 >= 0 else Y1 + g)
            bar = np.empty((9, 6 * len(text) + 1, 3), np.uint8)
            bar[:] = col
            ink = 0 if (299 * int(col[0]) + 587 * int(col[1]) + 114 * int(col[2])) // 1000 >= 128 else 255
            for k, ch in enumerate(text):
                bar[1:8, 1 + 6 * k:6 + 6 * k][glyphs[CHARS.index(ch)]] = ink
            x0, x1, y0, y1 = max(bx, 0), min(bx + bar.shape[1], W), max(by, 0), min(by + 9, H)
            if x0 < x1 and y0 < y1:
                img[y0:y1, x0:x1] = bar[y0 - by:y1 - by, x0 - bx:x1 - bx]
    return out


# ---- sheets ----------------------------------------------------------------------------------------------------------------

def _check_sheet(who, q_shape, s_shape, side, pad, pad_value):
    if len(q_shape) != 4 or q_shape[3] != 3 or len(s_shape) != 5 or s_shape[4] != 3 or s_shape[0] != q_shape[0]:
        raise ValueError("%s: query_rgb uint8 [N, H, W, 3] and supports_rgb uint8 [N, S, hs, ws, 3], got %s and %s"
                         % (who, tuple(q_shape), tuple(s_shape)))
    if min(q_shape[1:3]) < 1 or (s_shape[1] > 0 and min(s_shape[2:4]) < 1):
        raise ValueError("%s: empty images (%s, %s)" % (who, tuple(q_shape), tuple(s_shape)))
    if int(side) < 1 or int(pad) < 0 or not 0 <= int(pad_value) <= 255:
        raise ValueError("%s: side >= 1, pad >= 0 and pad_value in 0..255, got %s, %s, %s" % (who, side, pad, pad_value))
    if int(side) > q_shape[1]:
        raise ValueError("%s: side %d is larger than the query's height %d" % (who, side, q_shape[1]))


def sheet_geometry(H, W, S, side=160, pad=4):
    """-> (rows_per_col, cols, output width, [(x, y) top-left corner of shot s])"""
    rpc = max(1, (H + pad) // (side + pad))
    cols = -(-S // rpc)
    return rpc, cols, W + cols * (pad + side), [(W + pad + (s // rpc) * (side + pad), (s % rpc) * (side + pad))
                                                for s in range(S)]


def sheet(query_rgb, supports_rgb, side=160, pad=4, pad_value=255):
    """query_rgb uint8 [N, H, W, 3] and supports_rgb uint8 [N, S, hs, ws, 3] -> uint8 [N, H, W + cols * (pad + side), 3]:
    the query at the left, the shots to its right in columns of rows_per_col = max(1, (H + pad) // (side + pad)), shot s
    at (x = W + pad + (s // rows_per_col) * (side + pad), y = (s % rows_per_col) * (side + pad)), pad_value elsewhere.
    Each shot is resized to side x side with cv2.resize(INTER_LINEAR)'s rule as the input pipeline states it: sample
    position (d + 0.5) * src / side - 0.5 in float64, rounded to float32, floor, clamped ends. Interpolation per channel
    in fp32, in this order: h0 = p[y0][x0] * ax0 + p[y0][x1] * ax1, h1 = p[y1][x0] * ax0 + p[y1][x1] * ax1,
    v = h0 * ay0 + h1 * ay1 (no fused multiply-add), byte = trunc(clamp(v, 0, 255) + 0.5). One launch."""
    _cuda(query_rgb, "query_rgb", torch.uint8, "sheet")
    _cuda(supports_rgb, "supports_rgb", torch.uint8, "sheet")
    _check_sheet("sheet", query_rgb.shape, supports_rgb.shape, side, pad, pad_value)
    return ops.render_sheet(query_rgb.contiguous(), supports_rgb.contiguous(), int(side), int(pad), int(pad_value))


def _taps(n_dst, scale, n_src):
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= n_src - 1
    s[lo], f[lo] = 0, 0.0
    s[hi], f[hi] = n_src - 1, 0.0
    return s, np.minimum(s + 1, n_src - 1), (np.float32(1.0) - f).astype(np.float32), f.astype(np.float32)


def resize_numpy(shot, side):
    """one uint8 [hs, ws, 3] shot -> uint8 [side, side, 3] by `sheet`'s rule (numpy float32, the same operation order)"""
    src = np.asarray(shot, np.uint8).astype(np.float32)
    hs, ws = src.shape[:2]
    x0, x1, a0, a1 = _taps(side, ws / float(side), ws)
    y0, y1, b0, b1 = _taps(side, hs / float(side), hs)
    hor = src[:, x0] * a0[None, :, None] + src[:, x1] * a1[None, :, None]
    v = hor[y0] * b0[:, None, None] + hor[y1] * b1[:, None, None]
    return (np.minimum(np.maximum(v, np.float32(0)), np.float32(255)) + np.float32(0.5)).astype(np.uint8)


def sheet_numpy(query_rgb, supports_rgb, side=160, pad=4, pad_value=255):
    """`sheet` restated in numpy (host)"""
    q, sup = np.asarray(query_rgb, np.uint8), np.asarray(supports_rgb, np.uint8)
    _check_sheet("sheet_numpy", q.shape, sup.shape, side, pad, pad_value)
    N, H, W = q.shape[:3]
    S = sup.shape[1]
    _, _, out_w, corners = sheet_geometry(H, W, S, side, pad)
    out = np.full((N, H, out_w, 3), pad_value, np.uint8)
    out[:, :, :W] = q
    for n in range(N):
        for s, (x, y) in enumerate(corners):
            out[n, y:y + side, x:x + side] = resize_numpy(sup[n, s], side)
    return out


def _packed_layout(dets):
    """a ClassDetections / MergedDetections or a (packed, layout_dev) pair -> (packed [rows, 5], layout_dev)"""
    if hasattr(dets, "packed") and hasattr(dets, "layout_dev"):
        packed, layout = dets.packed, dets.layout_dev
    elif isinstance(dets, (tuple, list)) and len(dets) == 2 and all(torch.is_tensor(d) for d in dets):
        packed, layout = dets
    else:
        raise ValueError("prediction_sheet: dets must be a ClassDetections, a MergedDetections or a (packed, layout_dev) pair")
    if packed is None or layout is None:
        raise ValueError("prediction_sheet: the detections carry no device layout (detections_by_class(..., with_layout=True))")
    return packed.reshape(-1, packed.size(-1)), layout


def prediction_sheet(im_data, im_info, dets, supports, thickness=2, min_score=None, colors=None, color_index=None,
                     labels=True, top="first", side=160, pad=4, pad_value=255):
    """The README's prediction figure: im_data [N, 3, H, W] and supports [N, S, 3, hs, ws] as the model is fed, im_info
    [N, 3], dets a `ClassDetections` (detections_by_class(..., with_layout=True)), a `MergedDetections` or a
    (packed, layout_dev) pair -> uint8 [N, H, W + cols * (pad + side), 3]: `to_rgb` of the query with the detections drawn
    at scale im_info[:, 2] (`draw_boxes`), the shots beside it (`sheet`). Four launches, nothing read back."""
    packed, layout = _packed_layout(dets)
    _cuda(im_info, "im_info", torch.float32, "prediction_sheet")
    if im_data.dim() != 4 or supports.dim() != 5 or im_info.dim() != 2 or im_info.size(1) < 3 or im_info.size(0) != im_data.size(0):
        raise ValueError("prediction_sheet: im_data [N, 3, H, W], im_info [N, 3], supports [N, S, 3, hs, ws], got %s, %s, %s"
                         % (tuple(im_data.shape), tuple(im_info.shape), tuple(supports.shape)))
    canvas = to_rgb(im_data)
    draw_boxes(canvas, packed, layout, scale=im_info[:, 2].contiguous(), thickness=thickness, min_score=min_score,
               colors=colors, color_index=color_index, labels=labels, top=top)
    return sheet(canvas, to_rgb(supports), side, pad, pad_value)


def episode_sheet(im_data, gt_boxes, num_boxes, support_ims, shot, thickness=2, colors=None, labels=True, side=160, pad=4,
                  pad_value=255):
    """What FSODLogger._add_images shows of a training episode (fsod_logger.py:56-102): the ground-truth boxes
    (gt_boxes [N, K, 5], the first num_boxes[b] rows, class-0 rows left out) on the query, the first positive shot
    support_ims[:, 0] and the first negative one support_ims[:, shot] beside it (a one-way episode has no negative shot:
    the positive alone). The images are restored with cfg.PIXEL_MEANS -- true colours --, NOT min-max normalised per
    grid as the reference's make_grid(normalize=True) does."""
    if gt_boxes.dim() != 3 or gt_boxes.size(2) != 5 or support_ims.dim() != 5:
        raise ValueError("episode_sheet: gt_boxes [N, K, 5] and support_ims [N, S, 3, hs, ws], got %s and %s"
                         % (tuple(gt_boxes.shape), tuple(support_ims.shape)))
    picks = [0, int(shot)] if support_ims.size(1) > int(shot) > 0 else [0]
    canvas = to_rgb(im_data)
    draw_boxes(canvas, gt_boxes.contiguous().view(-1, 5), per_image=gt_boxes.size(1), num_boxes=num_boxes,
               thickness=thickness, colors=colors, labels=labels)
    shots = torch.stack([support_ims[:, s] for s in picks], 1)
    return sheet(canvas, to_rgb(shots), side, pad, pad_value)


# ---- writers: the only place where pixels go to the host -------------------------------------------------------------------

def _host_rgb(rgb, who):
    if torch.is_tensor(rgb):
        rgb = rgb.detach().cpu().numpy()
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError("%s: rgb must be a uint8 [H, W, 3] tensor or array, got %s %s" % (who, rgb.dtype, rgb.shape))
    return np.ascontiguousarray(rgb)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def png_bytes(rgb):
    """uint8 [H, W, 3] -> the bytes of an 8-bit RGB PNG: filter type 0 on every row, one zlib stream in one IDAT"""
    rgb = _host_rgb(rgb, "write_png")
    h, w, _ = rgb.shape
    raw = np.concatenate((np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)), 1).tobytes()
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(raw)) + _chunk(b"IEND", b""))


def write_png(path, rgb):
    """a uint8 [H, W, 3] tensor (device or host) or array -> an 8-bit RGB PNG file; the standard library only"""
    data = png_bytes(rgb)
    with open(path, "wb") as f:
        f.write(data)


def write_ppm(path, rgb):
    """a uint8 [H, W, 3] tensor (device or host) or array -> a binary PPM (P6) file"""
    rgb = _host_rgb(rgb, "write_ppm")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())
