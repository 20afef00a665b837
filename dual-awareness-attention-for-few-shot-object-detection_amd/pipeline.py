"""Episode input pipeline on the device.

Mirrors what the reference's loaders do per image on the CPU with cv2 / numpy:
  * `prep_im_for_blob`   lib/model/utils/blob.py:35-52 (called from roi_data_layer/minibatch.py:70-84)
  * `support_crop`       roi_data_layer/fs_loader.py:118-139 (crop the support box, fit it into target x target)
  * `crop_pad_chw`       fs_loader.py:186-280,318 (query crop window, ratio padding, permute(2, 0, 1))
  * `EpisodeHolders`     train.py:61-66,125-129 (persistent device holders the model is fed from)
  * `ImagePool`, `plan_episode`, `EpisodeAssembler`   fs_loader.py:81-325 for a whole batch: resident frames, one plan
                         made on the host, three launches (csrc/episode.hip), the same bits as the functions above
  * `color_matrix`, `draw_color_matrix`, the query keys target_size / crop / min_visible / color   training-time
                         augmentation, chosen per record on the host and evaluated by those launches (not in the reference)
  * `mosaic_query`, `paste_part`, `draw_mosaic`, `draw_paste`, the query keys parts / at   composed queries: mosaic,
                         copy-paste and random erasing as ordered parts painted into one holder image (not in the reference)
Raw uint8 RGB frames are uploaded once; everything else happens in HBM through libdana_hip.so. The data-dependent
host decisions (which crop window, which supports: np.random / random in fs_loader.py) stay on the host, as they
are in the reference."""
import ctypes

import numpy as np
import torch

from ._lib import lib
from .config import cfg
from .ops import _chk, _p, _stream


def cv_round(x):
    """cv2's saturate_cast<int>(double): round half to even (cvRound)"""
    return int(np.rint(x))


def prep_im_for_blob(im_rgb_u8, pixel_means=None, target_size=600, max_size=1000, flipped=False):
    """im_rgb_u8: uint8 [h][w][3] RGB on the device (what `imread` returns, minibatch.py:70) -> (fp32 [oh][ow][3] BGR,
    mean-subtracted, resized so that the SHORTER side is target_size; im_scale). max_size is ignored exactly as in
    blob.py:45-47 (the cap is commented out there)."""
    if im_rgb_u8.dtype != torch.uint8 or im_rgb_u8.dim() != 3 or im_rgb_u8.size(2) != 3 or not im_rgb_u8.is_cuda:
        raise RuntimeError("prep_im_for_blob: need a uint8 [h][w][3] HIP tensor")
    im = im_rgb_u8.contiguous()
    h, w = im.size(0), im.size(1)
    means = np.asarray(cfg.PIXEL_MEANS if pixel_means is None else pixel_means, dtype=np.float32).reshape(-1)
    im_scale = float(target_size) / float(min(h, w))
    oh, ow = cv_round(h * im_scale), cv_round(w * im_scale)
    out = torch.empty((oh, ow, 3), dtype=torch.float32, device=im.device)
    f3 = ctypes.c_float * 3
    lib().call("dana_prep_image", im.data_ptr(), h, w, w * 3, int(bool(flipped)),
               ctypes.cast(f3(*[float(m) for m in means[:3]]), ctypes.c_void_p), im_scale, _p(out), oh, ow, _stream())
    return out, im_scale


def support_crop(im_hwc, box_scaled, target_size=320, out=None):
    """fs_loader.py:118-139. im_hwc: prepared fp32 [h][w][3]; box_scaled: (x_min, y_min, x_max, y_max) already
    multiplied by the image's scale and cast to int16 by the caller. -> fp32 [3][target][target]"""
    _chk(im_hwc, "im_hwc")
    h, w = im_hwc.size(0), im_hwc.size(1)
    x_min, y_min, x_max, y_max = [int(v) for v in box_scaled]
    box_h, box_w = y_max - y_min, x_max - x_min
    if box_h > box_w:
        rw, rh = int(box_w * (float(target_size) / float(box_h))), target_size
    else:
        rw, rh = target_size, int(box_h * (float(target_size) / float(box_w)))
    if out is None:
        out = torch.empty((3, target_size, target_size), dtype=torch.float32, device=im_hwc.device)
    lib().call("dana_crop_resize_pad", _p(im_hwc), h, w, x_min, y_min, min(x_max, w - 1), min(y_max, h - 1), rw, rh,
               target_size, _p(out), _stream())
    return out


def crop_pad_chw(im_hwc, y_start, x_start, crop_h, crop_w, out_h, out_w, out=None):
    """fs_loader.py:186-280,318: data[:, y_s:y_s+crop_h, x_s:x_s+crop_w, :] zero-padded to [out_h][out_w], as CHW"""
    _chk(im_hwc, "im_hwc")
    if out is None:
        out = torch.empty((3, out_h, out_w), dtype=torch.float32, device=im_hwc.device)
    lib().call("dana_crop_pad_chw", _p(im_hwc), im_hwc.size(0), im_hwc.size(1), y_start, x_start, crop_h, crop_w,
               _p(out), out_h, out_w, _stream())
    return out


def pad_plan(data_h, data_w, ratio):
    """the padding branch of fs_loader.py:257-280 for an image that needs no crop: -> (out_h, out_w, copy_h, copy_w)"""
    if ratio < 1:
        return int(np.ceil(data_w / ratio)), data_w, data_h, data_w
    if ratio > 1:
        return data_h, int(np.ceil(data_h * ratio)), data_h, data_w
    t = min(data_h, data_w)
    return t, t, t, t


class EpisodeHolders:
    """train.py:61-66: the five persistent device tensors (im_data, im_info, gt_boxes, num_boxes, support_ims) one
    batch of episodes is assembled in; `put_*` write one episode's slice with the kernels above."""

    def __init__(self, batch, way, shot, height, width, device, support_size=320, max_num_box=None):
        nb = cfg.MAX_NUM_GT_BOXES if max_num_box is None else max_num_box
        self.im_data = torch.zeros((batch, 3, height, width), dtype=torch.float32, device=device)
        self.im_info = torch.zeros((batch, 3), dtype=torch.float32, device=device)
        self.gt_boxes = torch.zeros((batch, nb, 5), dtype=torch.float32, device=device)
        self.num_boxes = torch.zeros((batch,), dtype=torch.long, device=device)
        self.support_ims = torch.zeros((batch, way * shot, 3, support_size, support_size), dtype=torch.float32,
                                       device=device)
        self.support_size = support_size

    def put_query(self, b, im_hwc, im_scale, y_start=0, x_start=0, crop_h=None, crop_w=None):
        H, W = self.im_data.size(2), self.im_data.size(3)
        crop_h = im_hwc.size(0) - y_start if crop_h is None else crop_h
        crop_w = im_hwc.size(1) - x_start if crop_w is None else crop_w
        crop_pad_chw(im_hwc, y_start, x_start, min(crop_h, H), min(crop_w, W), H, W, out=self.im_data[b])
        self.im_info[b] = torch.tensor([float(H), float(W), float(im_scale)], device=self.im_info.device)

    def put_support(self, b, slot, im_hwc, box_scaled):
        support_crop(im_hwc, box_scaled, self.support_size, out=self.support_ims[b, slot])

    def put_boxes(self, b, boxes):
        """boxes: float [n][5] (already scaled / shifted / clamped / filtered like fs_loader.py:282-313)"""
        n = min(int(boxes.shape[0]), self.gt_boxes.size(1))
        self.gt_boxes[b].zero_()
        if n:
            self.gt_boxes[b, :n] = torch.as_tensor(boxes[:n], dtype=torch.float32).to(self.gt_boxes.device)
        self.num_boxes[b] = n

    def tensors(self):
        return self.im_data, self.im_info, self.gt_boxes, self.num_boxes, self.support_ims


# ---- a batch of episodes from a resident image pool (csrc/episode.hip) ---------------------------------------------------
# The raw frames stay on the device; per batch the host decides what the reference's loader decides with random / np.random
# (which supports, which crop start, which box order), `plan_episode` derives everything that follows from those choices,
# and `EpisodeAssembler.assemble` turns the plan into the holders' contents with one upload and three launches.

# plan records, in int32 words (the enums of csrc/episode.hip); doubles sit on even words
EP_QWORDS, EP_SWORDS = 16, 16
(Q_ROW, Q_NORDER, Q_SCALE, Q_INV, Q_YS, Q_XS, Q_COPY_H, Q_COPY_W, Q_CLAMP_X, Q_CLAMP_Y, Q_CLS,
 Q_ORDER_OFF, Q_OH, Q_OW) = 0, 1, 2, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15
S_ROW, S_INV, S_SX, S_SY, S_X0, S_Y0, S_CW, S_CH, S_RW, S_RH, S_OH, S_OW = 0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 14, 15
# augmentation record (the plan's third section, present only when something asks for it): float32 M[3][4], float32
# min_visible, flags
EP_AWORDS = 16
A_M, A_MIN_VISIBLE, A_FLAGS = 0, 12, 13
A_HAS_COLOR, A_HAS_VISIBLE = 1, 2
# composed section (the plan's last, present only when a query is composed): one header per query, then one table of
# `max_parts` part records per query. A part record starts like a query record and goes on with the destination, the word
# offset of its box order, its flags (A_HAS_COLOR) and float32 M[3][4]; words 28, 29 hold the prepared size for the host.
EP_CWORDS, EP_PWORDS, EP_MAX_PARTS = 8, 32, 16
C_NPARTS, C_CLS, C_MIN_VISIBLE, C_FLAGS = 0, 1, 2, 3
(P_ROW, P_NORDER, P_SCALE, P_INV, P_YS, P_XS, P_H, P_W, P_CLAMP_X, P_CLAMP_Y, P_DY, P_DX, P_ORDER_OFF, P_FLAGS, P_M, P_OH,
 P_OW) = 0, 1, 2, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 28, 29


class ImagePool:
    """Raw uint8 RGB frames of different sizes in ONE device byte buffer, with their annotations beside them. Each frame
    starts on a 16-byte boundary; its rows are packed (w * 3 bytes). A flipped roidb entry (imdb.append_flipped_images) is a
    row of its own that shares the pixel bytes of its twin and carries its own, already flipped boxes.
    device=None keeps the tables on the host only (what `plan_episode` reads); with a device, `freeze()` uploads the frames
    and the tables once."""

    def __init__(self, device=None):
        self.device = None if device is None else torch.device(device)
        self._frames = []  # (host array | device tensor, byte offset)
        self._rows = []    # (frame index, flipped, float32 [n][5] boxes)
        self._end = 0
        self.frozen = False

    @staticmethod
    def _boxes(boxes):
        if torch.is_tensor(boxes):
            boxes = boxes.detach().cpu().numpy()
        b = np.asarray(boxes, dtype=np.float32).reshape(-1, 5) if np.size(boxes) else np.zeros((0, 5), dtype=np.float32)
        return np.ascontiguousarray(b)

    def add(self, im_rgb_u8, boxes):
        """im_rgb_u8: uint8 [h][w][3] (host array or device tensor); boxes: float32 [n][5] (x1, y1, x2, y2, class), unscaled
        as in roidb['boxes'] / roidb['gt_classes'] -> the row index"""
        if self.frozen:
            raise RuntimeError("ImagePool.add: the pool is frozen")
        im = im_rgb_u8 if torch.is_tensor(im_rgb_u8) else np.asarray(im_rgb_u8)
        if im.dtype not in (torch.uint8, np.uint8) or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError("ImagePool.add: need a uint8 [h][w][3] image")
        self._frames.append((im, self._end))
        self._end = (self._end + im.shape[0] * im.shape[1] * 3 + 15) // 16 * 16
        self._rows.append((len(self._frames) - 1, 0, self._boxes(boxes)))
        return len(self._rows) - 1

    def add_flipped(self, row, boxes):
        """the horizontally flipped twin of `row` (no second copy of the pixels); boxes: the twin's, already flipped"""
        if self.frozen:
            raise RuntimeError("ImagePool.add_flipped: the pool is frozen")
        if not 0 <= int(row) < len(self._rows):
            raise IndexError("ImagePool.add_flipped: row %d outside [0, %d)" % (row, len(self._rows)))
        frame, flipped, _ = self._rows[int(row)]
        self._rows.append((frame, 1 - flipped, self._boxes(boxes)))
        return len(self._rows) - 1

    def freeze(self):
        if self.frozen:
            return self
        n = len(self._rows)
        self.offsets = np.array([self._frames[f][1] for f, _, _ in self._rows], dtype=np.int64)
        self.meta = np.zeros((n, 5), dtype=np.int32)  # h, w, flipped, first box, box count
        at = 0
        for r, (f, flipped, bx) in enumerate(self._rows):
            im = self._frames[f][0]
            self.meta[r] = (im.shape[0], im.shape[1], flipped, at, bx.shape[0])
            at += bx.shape[0]
        self.boxes = np.concatenate([bx for _, _, bx in self._rows] + [np.zeros((0, 5), dtype=np.float32)], axis=0)
        self.frozen = True
        if self.device is not None:
            staged = np.zeros((max(self._end, 16),), dtype=np.uint8)
            for im, off in self._frames:
                if not torch.is_tensor(im):
                    staged[off:off + im.size] = np.ascontiguousarray(im).reshape(-1)
            self.data = torch.from_numpy(staged).to(self.device)
            for im, off in self._frames:
                if torch.is_tensor(im):
                    self.data[off:off + im.numel()] = im.to(self.device).reshape(-1)
            self.d_offsets = torch.from_numpy(self.offsets).to(self.device)
            self.d_meta = torch.from_numpy(self.meta).to(self.device)
            self.d_boxes = torch.from_numpy(self.boxes if len(self.boxes) else np.zeros((1, 5), np.float32)).to(self.device)
        self._frames = [(None, off) for _, off in self._frames]
        return self

    def __len__(self):
        return len(self._rows)

    @property
    def nbytes(self):
        """bytes of the frame buffer (alignment padding included)"""
        return int(self._end)

    def row_boxes(self, row):
        return self._rows[row][2]

    def frame_of(self, row):
        """the index of the frame whose pixels `row` reads: a flipped twin has its twin's (and `meta[row, 2]` = 1 - its
        twin's flipped bit; `meta[row, :2]` is the frame's h, w)"""
        return self._rows[int(row)][0]


class EpisodePlan:
    """One batch of episodes as the device reads it: `words` (int32) = `batch` query records, `n_supports` support
    records, the queries' box orders. `queries` / `supports` are the same records as dicts, for the host.
    `augmented`: the words end with a third section at `a_off` (an even word), one augmentation record per query, then one
    per support; `EpisodeAssembler` then runs the augmented launches. a_off is None for a plan that asks for none.
    `composed`: a query carries `parts`; the words end with the composed section at `c_off` (an even word): `batch` headers,
    then `batch` tables of `max_parts` part records, then the parts' box orders. `EpisodeAssembler` then runs the composed
    query and box launches for the whole batch (a query that is not composed is one part at (0, 0) in that section, built
    from its own record), and the section in front of it is what the plan would have without composed queries; in a
    composed plan `augmented` says only whether a support carries a colour map. c_off is None for any other plan."""

    def __init__(self, words, queries, supports, holder_hw, a_off=None, c_off=None, max_parts=0):
        self.words, self.queries, self.supports, self.holder_hw = words, queries, supports, holder_hw
        self.batch, self.n_supports = len(queries), len(supports)
        self.q_off, self.s_off = 0, len(queries) * EP_QWORDS
        self.augmented, self.a_off = a_off is not None, a_off
        self.composed, self.c_off, self.max_parts = c_off is not None, c_off, int(max_parts)

    def boxes_numpy(self, pool, max_num_box):
        """`episode_boxes_numpy` per query (`composed_boxes_numpy` for a composed one) -> (gt_boxes [B][max][5],
        num_boxes [B], all_cls_gt_boxes, all_cls_num_boxes)"""
        per = [composed_boxes_numpy([dict(p, boxes=None if p["row"] < 0 else pool.row_boxes(p["row"])) for p in q["parts"]],
                                    q["pos_cls"], max_num_box, min_visible=q.get("min_visible") or 0.0) if "parts" in q else
               episode_boxes_numpy(pool.row_boxes(q["row"]), q["order"], q["im_scale"], q["x_s"], q["y_s"], q["clamp_x"],
                                   q["clamp_y"], q["pos_cls"], max_num_box, min_visible=q.get("min_visible") or 0.0)
               for q in self.queries]
        return (np.stack([p[0] for p in per]), np.array([p[1] for p in per], dtype=np.int64),
                np.stack([p[2] for p in per]), np.array([p[3] for p in per], dtype=np.int64))


def _host_only(name, v):
    if getattr(v, "is_cuda", False):
        raise ValueError("plan_episode: %s is a device tensor; the plan is made on the host" % name)
    return v


def _pool_row(pool, row):
    if not pool.frozen:
        raise RuntimeError("plan_episode: freeze() the pool first")
    row = int(_host_only("row", row))
    if not 0 <= row < len(pool):
        raise IndexError("plan_episode: pool row %d outside [0, %d)" % (row, len(pool)))
    h, w = int(pool.meta[row, 0]), int(pool.meta[row, 1])
    return row, h, w


def color_matrix(brightness=0.0, contrast=1.0, saturation=1.0, hue=0.0, pivot=128.0):
    """The colour distortions of a training loader as ONE affine map of an RGB pixel -> float32 [3][4], rows R, G, B of the
    distorted pixel, columns r, g, b of the source, the offset in column 3. Applied in this order: brightness (v + b),
    contrast about a fixed pivot (c * (v - pivot) + pivot), saturation (s * v + (1 - s) * luma(v), luma weights 0.299 /
    0.587 / 0.114), hue (a rotation by `hue` degrees of the I, Q plane of YIQ). Composed in float64 and rounded once; a
    component at its neutral value contributes nothing, so `color_matrix()` is the identity exactly. Not in the reference."""
    m = np.eye(4, dtype=np.float64)
    luma = np.array([0.299, 0.587, 0.114], dtype=np.float64)
    step = np.eye(4, dtype=np.float64)
    if brightness != 0.0:
        step[:3, 3] = float(brightness)
        m = step @ m
    if contrast != 1.0:
        step = np.eye(4, dtype=np.float64)
        step[:3, :3] *= float(contrast)
        step[:3, 3] = (1.0 - float(contrast)) * float(pivot)
        m = step @ m
    if saturation != 1.0:
        step = np.eye(4, dtype=np.float64)
        step[:3, :3] = float(saturation) * np.eye(3) + (1.0 - float(saturation)) * np.tile(luma, (3, 1))
        m = step @ m
    if hue != 0.0:
        to_yiq = np.array([luma, [0.595716, -0.274453, -0.321263], [0.211456, -0.522591, 0.311135]], dtype=np.float64)
        a = np.deg2rad(float(hue))
        rot = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]], dtype=np.float64)
        step = np.eye(4, dtype=np.float64)
        step[:3, :3] = np.linalg.solve(to_yiq, rot @ to_yiq)
        m = step @ m
    return np.ascontiguousarray(m[:3], dtype=np.float32)


def draw_color_params(rng, brightness=32, contrast=(0.5, 1.5), saturation=(0.5, 1.5), hue=18, p=0.5):
    """One draw of the four components from a `numpy.random.Generator`, on the host: brightness uniform in [-b, b],
    contrast and saturation uniform in their (lo, hi), hue uniform in [-hue, hue] degrees, each applied with probability p
    and neutral otherwise. Eight numbers are drawn whatever the outcome, so the stream after a draw does not depend on it.
    -> the keyword arguments of `color_matrix`"""
    gate = rng.random(4) < float(p)
    u = rng.random(4)
    return dict(brightness=float((2.0 * u[0] - 1.0) * brightness) if gate[0] else 0.0,
                contrast=float(contrast[0] + u[1] * (contrast[1] - contrast[0])) if gate[1] else 1.0,
                saturation=float(saturation[0] + u[2] * (saturation[1] - saturation[0])) if gate[2] else 1.0,
                hue=float((2.0 * u[3] - 1.0) * hue) if gate[3] else 0.0)


def draw_color_matrix(rng, brightness=32, contrast=(0.5, 1.5), saturation=(0.5, 1.5), hue=18, p=0.5):
    """`color_matrix` of one `draw_color_params` draw: deterministic under the generator's seed"""
    return color_matrix(**draw_color_params(rng, brightness, contrast, saturation, hue, p))


def _prepared_hw(pool, row, target_size):
    row, h, w = _pool_row(pool, row)
    im_scale = float(target_size) / float(min(h, w))
    return row, im_scale, cv_round(h * im_scale), cv_round(w * im_scale)


def mosaic_query(pool, rows, center, holder_hw, target_size=600, pos_cls=1, min_visible=0.5, colors=None, starts=None):
    """The composed query of a four-image mosaic, host only. rows: the pool rows of the top-left, top-right, bottom-left
    and bottom-right quadrant; center = (cy, cx) with 0 < cy < H, 0 < cx < W: the quadrants are [0, cy) / [cy, H) by
    [0, cx) / [cx, W) and tile the holder exactly. target_size: one scale or one per row. Each part is a window of its
    prepared image as large as its quadrant; starts: its (y, x) per part (None: the corner of the image that touches the
    centre, i.e. the top-left part ends with its image's last row and column). An image whose prepared size does not cover
    its quadrant is refused. colors: one map (or None) per part. -> dict(parts=[4 parts], pos_cls, min_visible) for
    `plan_episode`. Set min_visible: without it a box the window cuts down to a sliver stays."""
    H, W = int(holder_hw[0]), int(holder_hw[1])
    cy, cx = int(center[0]), int(center[1])
    if len(rows) != 4:
        raise ValueError("mosaic_query: needs four rows, got %d" % len(rows))
    if not (0 < cy < H and 0 < cx < W):
        raise ValueError("mosaic_query: centre (%d, %d) leaves no room for four quadrants in %d x %d" % (cy, cx, H, W))
    sizes = list(target_size) if np.ndim(target_size) else [target_size] * 4
    quads = [(0, 0, cy, cx), (0, cx, cy, W - cx), (cy, 0, H - cy, cx), (cy, cx, H - cy, W - cx)]
    parts = []
    for k, (dy, dx, qh, qw) in enumerate(quads):
        row, _, oh, ow = _prepared_hw(pool, rows[k], sizes[k])
        if qh > oh or qw > ow:
            raise ValueError("mosaic_query: row %d prepared to %d x %d does not cover its %d x %d quadrant" % (row, oh, ow, qh, qw))
        start = None if starts is None else starts[k]
        y, x = ((oh - qh) * (k < 2), (ow - qw) * (k % 2 == 0)) if start is None else (int(start[0]), int(start[1]))
        part = dict(row=row, crop=(y, x, qh, qw), at=(dy, dx), target_size=sizes[k])
        if colors is not None and colors[k] is not None:
            part["color"] = colors[k]
        parts.append(part)
    return dict(parts=parts, pos_cls=pos_cls, min_visible=min_visible)


def draw_mosaic(rng, pool, rows, holder_hw, target_size=600, center=(0.25, 0.75), **kw):
    """One mosaic from a `numpy.random.Generator`, on the host: the centre uniform in `center` (fractions of H and of W),
    each part's window uniform over the positions its prepared image allows. Ten numbers are drawn whatever the outcome.
    -> `mosaic_query(...)`, or None where a row's prepared image does not cover its quadrant"""
    u = rng.random(10)
    H, W = int(holder_hw[0]), int(holder_hw[1])
    cy = min(max(int(H * (center[0] + u[0] * (center[1] - center[0]))), 1), H - 1)
    cx = min(max(int(W * (center[0] + u[1] * (center[1] - center[0]))), 1), W - 1)
    sizes = list(target_size) if np.ndim(target_size) else [target_size] * 4
    quads = [(cy, cx), (cy, W - cx), (H - cy, cx), (H - cy, W - cx)]
    starts = []
    for k, (qh, qw) in enumerate(quads):
        _, _, oh, ow = _prepared_hw(pool, rows[k], sizes[k])
        if qh > oh or qw > ow:
            return None
        starts.append((min(int(u[2 + 2 * k] * (oh - qh + 1)), oh - qh), min(int(u[3 + 2 * k] * (ow - qw + 1)), ow - qw)))
    return mosaic_query(pool, rows, (cy, cx), holder_hw, target_size=sizes, starts=starts, **kw)


def paste_part(pool, row, box_index, at, target_size=600, margin=0, color=None):
    """The part that pastes ONE stored box of `row`, host only: the window of the prepared image around box `box_index`
    (its scaled corners rounded outwards, `margin` prepared pixels more on every side, cut at the image), painted at
    at = (dy, dx), carrying only that box (order = [box_index]). -> a part dict for q["parts"]"""
    row, im_scale, oh, ow = _prepared_hw(pool, row, target_size)
    boxes = pool.row_boxes(row)
    k = int(box_index)
    if not 0 <= k < len(boxes):
        raise ValueError("paste_part: row %d has no box %d" % (row, k))
    x1, y1, x2, y2 = [float(v) * im_scale for v in boxes[k, :4]]
    m = int(margin)
    x0, y0 = max(int(np.floor(x1)) - m, 0), max(int(np.floor(y1)) - m, 0)
    xe, ye = min(int(np.ceil(x2)) + m, ow - 1), min(int(np.ceil(y2)) + m, oh - 1)
    if xe < x0 or ye < y0:
        raise ValueError("paste_part: box %d of row %d lies outside its image" % (k, row))
    part = dict(row=row, crop=(y0, x0, ye - y0 + 1, xe - x0 + 1), at=(int(at[0]), int(at[1])), target_size=target_size, order=[k])
    if color is not None:
        part["color"] = color
    return part


def draw_paste(rng, pool, row, box_index, holder_hw, target_size=600, margin=0, color=None):
    """`paste_part` at a destination drawn uniformly over the positions at which the window stays inside the holder. Two
    numbers are drawn whatever the outcome. -> the part, or None where the window is larger than the holder"""
    u = rng.random(2)
    part = paste_part(pool, row, box_index, (0, 0), target_size, margin, color)
    room_y, room_x = int(holder_hw[0]) - part["crop"][2], int(holder_hw[1]) - part["crop"][3]
    if room_y < 0 or room_x < 0:
        return None
    part["at"] = (min(int(u[0] * (room_y + 1)), room_y), min(int(u[1] * (room_x + 1)), room_x))
    return part


def apply_color_numpy(im_rgb_u8, m):
    """The colour map as the kernels of csrc/episode.hip evaluate it at a source tap, for a whole frame, in numpy: float32,
    ((M[j][0]*r + M[j][1]*g) + M[j][2]*b) + M[j][3], clamped to [0, 255] -> float32 [h][w][3] RGB. The distorted image is
    never rounded to uint8: that rounding is defined away."""
    im = np.asarray(im_rgb_u8).astype(np.float32)
    m = np.asarray(m, dtype=np.float32).reshape(3, 4)
    r, g, b = im[..., 0], im[..., 1], im[..., 2]
    d = np.stack([((m[j, 0] * r + m[j, 1] * g) + m[j, 2] * b) + m[j, 3] for j in range(3)], axis=-1)
    return np.minimum(np.maximum(d, np.float32(0)), np.float32(255)).astype(np.float32)


def _color(name, m):
    """a caller's colour map, checked -> float32 [3][4] (None stays None: no map)"""
    if m is None:
        return None
    m = np.asarray(_host_only(name, m))
    if m.shape != (3, 4):
        raise ValueError("plan_episode: %s must be a [3][4] matrix, got shape %s" % (name, tuple(m.shape)))
    with np.errstate(over="ignore"):
        m = np.ascontiguousarray(m, dtype=np.float32)
    if not np.isfinite(m).all():
        raise ValueError("plan_episode: %s is not finite" % name)
    return m


def _plan_support(pool, row, box, target_size, support_size):
    row, h, w = _pool_row(pool, row)
    im_scale = float(target_size) / float(min(h, w))  # blob.py:45
    oh, ow = cv_round(h * im_scale), cv_round(w * im_scale)
    scaled = np.asarray(_host_only("box", box), dtype=np.float32).reshape(-1)[:4] * np.float32(im_scale)
    if not (np.abs(scaled) < 32768).all():
        raise ValueError("plan_episode: support box %s of row %d does not fit int16 after scaling" % (list(box), row))
    x_min, y_min, x_max, y_max = [int(v) for v in scaled.astype(np.int16)]  # fs_loader.py:120
    box_h, box_w = y_max - y_min, x_max - x_min
    x_lim, y_lim = min(x_max, ow - 1), min(y_max, oh - 1)  # the slice [min : max + 1] ends with the image
    if x_min < 0 or y_min < 0 or x_lim < x_min or y_lim < y_min:
        raise ValueError("plan_episode: support box %s lies outside its image (row %d, prepared %d x %d)"
                         % ((x_min, y_min, x_max, y_max), row, oh, ow))
    if box_h > box_w:  # fs_loader.py:126-133
        rw, rh = int(box_w * (float(support_size) / float(box_h))), support_size
    else:
        rw, rh = support_size, (int(box_h * (float(support_size) / float(box_w))) if box_w > 0 else 0)
    if rw <= 0 or rh <= 0:
        raise ValueError("plan_episode: support box %s resizes to %d x %d" % ((x_min, y_min, x_max, y_max), rw, rh))
    cw, ch = x_lim - x_min + 1, y_lim - y_min + 1
    return dict(row=row, im_scale=im_scale, oh=oh, ow=ow, x_min=x_min, y_min=y_min, x_max=x_lim, y_max=y_lim, rw=rw, rh=rh,
                cw=cw, ch=ch)


QUERY_KEYS = ("row", "ratio", "pos_cls", "order", "need_crop", "crop_start", "target_size", "crop", "min_visible", "color",
              "at", "parts")
AUGMENT_KEYS = ("min_visible", "color")  # a query that carries one of these (not None) makes the plan an augmented one
COMPOSE_KEYS = ("at", "parts")  # a query that carries one of these (not None) is composed, and so is the plan
PART_KEYS = ("row", "crop", "at", "target_size", "color", "order", "erase")


def _rect(name, v, n):
    v = np.asarray(_host_only(name, v)).reshape(-1)
    if v.size != n:
        raise ValueError("plan_episode: %s must have %d entries, got %r" % (name, n, v.tolist()))
    return [int(x) for x in v]


def _plan_part(pool, part, k, holder_hw, target_size):
    """one part of a composed query -> its host record: the record of a `crop` query plus the destination (dy, dx) and the
    painted size (h, w); an erase part has row -1, no boxes and no source"""
    H, W = int(holder_hw[0]), int(holder_hw[1])
    for key in part:
        if key not in PART_KEYS:
            raise ValueError("plan_episode: unknown key %r in part %d (known: %s)" % (key, k, ", ".join(PART_KEYS)))
    if part.get("erase") is not None:
        if any(part.get(key) is not None for key in PART_KEYS if key != "erase"):
            raise ValueError("plan_episode: part %d gives erase together with %s" %
                             (k, ", ".join(key for key in PART_KEYS if key != "erase" and part.get(key) is not None)))
        dy, dx, h, w = _rect("erase", part["erase"], 4)
        rec = dict(row=-1, im_scale=1.0, oh=h, ow=w, y_s=0, x_s=0, order=np.zeros((0,), dtype=np.int32), color=None, erase=True)
    else:
        if part.get("row") is None or part.get("crop") is None or part.get("at") is None:
            raise ValueError("plan_episode: part %d needs row, crop and at (or erase)" % k)
        dy, dx = _rect("at", part["at"], 2)
        r = _plan_query(pool, dict(row=part["row"], crop=part["crop"], pos_cls=0, target_size=part.get("target_size"),
                                   color=part.get("color"), order=part.get("order")), (1 << 30, 1 << 30), target_size)
        h, w = r["out_h"], r["out_w"]
        rec = dict({key: r[key] for key in ("row", "im_scale", "oh", "ow", "y_s", "x_s", "order", "color")}, erase=False)
    if h < 1 or w < 1 or dy < 0 or dx < 0 or dy + h > H or dx + w > W:
        raise ValueError("plan_episode: part %d's destination (y %d, x %d, %d x %d) leaves the holder (%d x %d)"
                         % (k, dy, dx, h, w, H, W))
    return dict(rec, h=h, w=w, clamp_x=w - 1, clamp_y=h - 1, dy=dy, dx=dx)


def _plan_composed(pool, q, holder_hw, target_size):
    """a query with `at` (itself the only part) or `parts` -> its host record: part 0's numbers where a query record has
    them (what im_info reads), an empty box order of its own, and `parts`"""
    for key in ("ratio", "need_crop", "crop_start"):
        if q.get(key) is not None and q.get(key) is not False:
            raise ValueError("plan_episode: a composed query places windows (crop, at); it cannot carry %s" % key)
    if q.get("parts") is not None:
        for key in PART_KEYS:
            if q.get(key) is not None:
                raise ValueError("plan_episode: a query with parts cannot carry %s of its own; it belongs to a part" % key)
        parts = list(_host_only("parts", q["parts"]))
    else:
        parts = [{key: q[key] for key in PART_KEYS if q.get(key) is not None}]
    if not 1 <= len(parts) <= EP_MAX_PARTS:
        raise ValueError("plan_episode: a composed query has 1 to %d parts, got %d" % (EP_MAX_PARTS, len(parts)))
    recs = [_plan_part(pool, part, k, holder_hw, target_size) for k, part in enumerate(parts)]
    min_visible = q.get("min_visible")
    if min_visible is not None:
        min_visible = float(_host_only("min_visible", min_visible))
        if not 0.0 <= min_visible <= 1.0:
            raise ValueError("plan_episode: min_visible of a composed query must lie in [0, 1], got %r" % min_visible)
    head = {key: recs[0][key] for key in ("row", "im_scale", "oh", "ow", "y_s", "x_s", "clamp_x", "clamp_y")}
    head.update(copy_h=recs[0]["h"], copy_w=recs[0]["w"], out_h=recs[0]["h"], out_w=recs[0]["w"])
    return dict(head, pos_cls=int(_host_only("pos_cls", q["pos_cls"])), order=np.zeros((0,), dtype=np.int32), color=None,
                min_visible=min_visible, parts=recs)


def _plan_query(pool, q, holder_hw, target_size):
    for key in q:
        if key not in QUERY_KEYS:
            raise ValueError("plan_episode: unknown key %r in a query (known: %s)" % (key, ", ".join(QUERY_KEYS)))
    if q.get("at") is not None or q.get("parts") is not None:  # COMPOSE_KEYS
        return _plan_composed(pool, q, holder_hw, target_size)
    row, h, w = _pool_row(pool, q["row"])
    if q.get("target_size") is not None:  # this query's own scale: multi-scale training (cfg.TRAIN.SCALES)
        target_size = float(_host_only("target_size", q["target_size"]))
        if not target_size > 0:
            raise ValueError("plan_episode: target_size of row %d must be positive, got %r" % (row, target_size))
    im_scale = float(target_size) / float(min(h, w))
    oh, ow = cv_round(h * im_scale), cv_round(w * im_scale)
    color = _color("color", q.get("color"))
    min_visible = q.get("min_visible")
    if min_visible is not None:
        min_visible = float(_host_only("min_visible", min_visible))
        if not 0.0 <= min_visible <= 1.0:
            raise ValueError("plan_episode: min_visible of row %d must lie in [0, 1], got %r" % (row, min_visible))
    if q.get("crop") is not None:
        # a free window of the prepared image in place of the ratio crop, with the loader's own convention for a crop
        # (fs_loader.py:215-220, 251-255): shift by the start, clamp to [0, size - 1]. No ratio padding follows.
        if q.get("need_crop", False) or q.get("crop_start") is not None:
            raise ValueError("plan_episode: row %d gives both crop and need_crop / crop_start" % row)
        win = np.asarray(_host_only("crop", q["crop"])).reshape(-1)
        if win.size != 4:
            raise ValueError("plan_episode: crop must be (y, x, h, w), got %r" % (q["crop"],))
        y_s, x_s, ch, cw = [int(v) for v in win]
        if y_s < 0 or x_s < 0 or ch < 1 or cw < 1 or y_s + ch > oh or x_s + cw > ow:
            raise ValueError("plan_episode: crop window (y %d, x %d, %d x %d) leaves the prepared image (%d x %d) of row %d"
                             % (y_s, x_s, ch, cw, oh, ow, row))
        return dict(row=row, im_scale=im_scale, oh=oh, ow=ow, y_s=y_s, x_s=x_s, copy_h=min(ch, int(holder_hw[0])),
                    copy_w=min(cw, int(holder_hw[1])), out_h=ch, out_w=cw, clamp_x=cw - 1, clamp_y=ch - 1,
                    pos_cls=int(_host_only("pos_cls", q["pos_cls"])), order=_box_order(pool, row, q), color=color,
                    min_visible=min_visible)
    ratio = float(_host_only("ratio", q["ratio"]))
    data_h, data_w, y_s, x_s, clamp_x, clamp_y = oh, ow, 0, 0, -1, -1
    if q.get("need_crop", False):
        start = int(_host_only("crop_start", q.get("crop_start", 0)))
        if ratio < 1:  # fs_loader.py:187-220: crop the height
            trim = min(int(np.floor(data_w / ratio)), data_h)
            y_s, data_h, clamp_y = start, trim, trim - 1
        else:  # :222-255: crop the width
            trim = min(int(np.ceil(data_h * ratio)), data_w)
            x_s, data_w, clamp_x = start, trim, trim - 1
        if start < 0 or y_s + data_h > oh or x_s + data_w > ow:
            raise ValueError("plan_episode: crop window (start %d, size %d) leaves the prepared image (%d x %d) of row %d"
                             % (start, trim, oh, ow, row))
    out_h, out_w, copy_h, copy_w = pad_plan(data_h, data_w, ratio)  # :257-283
    if ratio == 1:
        clamp_x = copy_w if clamp_x < 0 else min(clamp_x, copy_w)  # :281 (after the crop's clamp, where both apply)
        clamp_y = copy_h if clamp_y < 0 else min(clamp_y, copy_h)
    if copy_h > holder_hw[0] or copy_w > holder_hw[1]:
        raise ValueError("plan_episode: copy window %d x %d of row %d is larger than the holder (%d x %d)"
                         % (copy_h, copy_w, row, holder_hw[0], holder_hw[1]))
    order = _box_order(pool, row, q)
    return dict(row=row, im_scale=im_scale, oh=oh, ow=ow, y_s=y_s, x_s=x_s, copy_h=copy_h, copy_w=copy_w, out_h=out_h,
                out_w=out_w, clamp_x=clamp_x, clamp_y=clamp_y, pos_cls=int(_host_only("pos_cls", q["pos_cls"])), order=order,
                color=color, min_visible=min_visible)


def _box_order(pool, row, q):
    n_box = int(pool.meta[row, 4])
    order = q.get("order")
    order = np.arange(n_box, dtype=np.int32) if order is None else np.asarray(_host_only("order", order)).astype(np.int32).reshape(-1)
    if len(order) and (order.min() < 0 or order.max() >= n_box):
        raise ValueError("plan_episode: box order of row %d names a box outside [0, %d)" % (row, n_box))
    return order


def _aug_offset(qs, ss):
    """the word at which the augmentation section starts: behind the box orders, on an even word"""
    n = len(qs) * EP_QWORDS + len(ss) * EP_SWORDS + sum(len(q["order"]) for q in qs)
    return n + (n & 1)


def _pack_plan(qs, ss, augmented=False):
    """the host records of `_plan_query` / `_plan_support` -> the int32 words the kernels of csrc/episode.hip read.
    augmented: the words go on to `_aug_offset(qs, ss)` and carry one augmentation record per query, then one per support
    (a record without a colour map holds the identity and no A_HAS_COLOR; min_visible > 0 sets A_HAS_VISIBLE)"""
    n_rec = len(qs) * EP_QWORDS + len(ss) * EP_SWORDS
    n_words = n_rec + sum(len(q["order"]) for q in qs)
    a_off = _aug_offset(qs, ss)
    words = np.zeros((a_off + (len(qs) + len(ss)) * EP_AWORDS if augmented else n_words,), dtype=np.int32)
    if augmented:
        f32 = words.view(np.float32)
        for k, rec in enumerate(list(qs) + list(ss)):
            o = a_off + k * EP_AWORDS
            color, f = rec.get("color"), rec.get("min_visible") or 0.0
            f32[o + A_M:o + A_M + 12] = (np.eye(3, 4, dtype=np.float32) if color is None else color).reshape(-1)
            f32[o + A_MIN_VISIBLE] = f
            words[o + A_FLAGS] = (A_HAS_COLOR if color is not None else 0) | (A_HAS_VISIBLE if f > 0 else 0)
    f64 = words[:n_rec].view(np.float64)  # word 2k <-> double k
    at = n_rec
    for b, q in enumerate(qs):
        o = b * EP_QWORDS
        words[o + Q_ROW], words[o + Q_NORDER] = q["row"], len(q["order"])
        f64[(o + Q_SCALE) // 2], f64[(o + Q_INV) // 2] = q["im_scale"], 1.0 / q["im_scale"]
        words[o + Q_YS:o + Q_YS + 4] = (q["y_s"], q["x_s"], q["copy_h"], q["copy_w"])
        words[o + Q_CLAMP_X:o + Q_CLAMP_X + 6] = (q["clamp_x"], q["clamp_y"], q["pos_cls"], at, q["oh"], q["ow"])
        words[at:at + len(q["order"])] = q["order"]
        at += len(q["order"])
    for n, s in enumerate(ss):
        o = len(qs) * EP_QWORDS + n * EP_SWORDS
        words[o + S_ROW] = s["row"]
        # cv2.resize(fx, fy) samples at 1 / fx, cv2.resize(dsize) at src / dst (csrc/pipeline.hip)
        f64[(o + S_INV) // 2], f64[(o + S_SX) // 2], f64[(o + S_SY) // 2] = 1.0 / s["im_scale"], s["cw"] / s["rw"], s["ch"] / s["rh"]
        words[o + S_X0:o + S_X0 + 8] = (s["x_min"], s["y_min"], s["cw"], s["ch"], s["rw"], s["rh"], s["oh"], s["ow"])
    return words


def _pack_composed(words, qs):
    """the words of `_pack_plan` + the composed section behind them, on an even word -> (words, c_off, max_parts).
    Headers, then one table of max_parts part records per query (unused records stay zero), then the parts' box orders.
    A query without `parts` becomes one part at (0, 0) made of its own record, its box order left where it is."""
    B = len(qs)
    max_parts = max(len(q.get("parts", (None,))) for q in qs)
    c_off = int(words.size) + (int(words.size) & 1)
    p_off = c_off + B * EP_CWORDS
    o_off = p_off + B * max_parts * EP_PWORDS
    out = np.zeros((o_off + sum(len(p["order"]) for q in qs for p in q.get("parts", ())),), dtype=np.int32)
    out[:words.size] = words
    f32, f64 = out.view(np.float32), out[:o_off].view(np.float64)
    at = o_off
    for b, q in enumerate(qs):
        o = c_off + b * EP_CWORDS
        f = q.get("min_visible") or 0.0
        parts = q.get("parts")
        if parts is None:  # its 16-word record says where its order is
            parts = [dict(q, h=q["copy_h"], w=q["copy_w"], dy=0, dx=0, order_off=int(words[b * EP_QWORDS + Q_ORDER_OFF]))]
        out[o + C_NPARTS], out[o + C_CLS], out[o + C_FLAGS] = len(parts), q["pos_cls"], (A_HAS_VISIBLE if f > 0 else 0)
        f32[o + C_MIN_VISIBLE] = f
        for k, p in enumerate(parts):
            o = p_off + (b * max_parts + k) * EP_PWORDS
            order_off = p.get("order_off")
            if order_off is None:
                order_off = at
                out[at:at + len(p["order"])] = p["order"]
                at += len(p["order"])
            out[o + P_ROW], out[o + P_NORDER] = p["row"], len(p["order"])
            f64[(o + P_SCALE) // 2], f64[(o + P_INV) // 2] = p["im_scale"], 1.0 / p["im_scale"]
            out[o + P_YS:o + P_YS + 10] = (p["y_s"], p["x_s"], p["h"], p["w"], p["clamp_x"], p["clamp_y"], p["dy"], p["dx"],
                                           order_off, A_HAS_COLOR if p.get("color") is not None else 0)
            f32[o + P_M:o + P_M + 12] = (np.eye(3, 4, dtype=np.float32) if p.get("color") is None else p["color"]).reshape(-1)
            out[o + P_OH], out[o + P_OW] = p["oh"], p["ow"]
    return out, c_off, max_parts


def plan_episode(pool, queries, supports=(), holder_hw=None, target_size=600, support_size=320):
    """Host only. queries: one dict per batch item with the loader's choices -- row, ratio (ratio_list_batch[index]),
    pos_cls, and optionally order (the shuffled box order of fs_loader.py:183; default: as stored), need_crop with
    crop_start (the y_s / x_s drawn at :186-255). supports: (row, box) per support slot, batch-major ([b][way * shot]
    flattened), box = the support_db entry's unscaled (x1, y1, x2, y2). holder_hw: (H, W) of the holders' im_data.
    -> EpisodePlan with everything that follows deterministically: scales, prepared sizes, copy windows, clamp limits, the
    int16 support boxes and their resized sizes.
    Training-time augmentation (not in the reference; the draws stay on the host, e.g. `draw_color_matrix`), per record:
      q["target_size"]  this query's own scale in place of `target_size` (multi-scale training)
      q["crop"]         (y, x, h, w) in prepared pixels: a free window in place of need_crop / crop_start; boxes are shifted
                        by its start and clamped to [0, w - 1] x [0, h - 1]; no ratio padding (`ratio` is not read)
      q["min_visible"]  f in [0, 1]: a box stays only if the shift and the clamp leave at least f of its area (0: no rule)
      q["color"]        a float [3][4] map of the source's RGB (`color_matrix`), applied to every source tap
      supports          (row, box, color) in place of (row, box)
    A plan in which a query carries min_visible or color, or a support a color, is `augmented`: its words end with the
    augmentation section and `EpisodeAssembler` runs the augmented launches. Any other plan has the words it always had.
    Composed queries (not in the reference; `mosaic_query`, `paste_part`, `draw_mosaic`, `draw_paste` build them): an ordered
    list of 1 to 16 parts painted into the holder, later parts over earlier ones, their boxes gathered in that order.
      q["parts"]        [dict(row, crop, at, target_size?, color?, order?) | dict(erase=(dy, dx, h, w))]: a part is the
                        window `crop` of its row's prepared image, painted with its top-left corner at at = (dy, dx); the
                        destination rectangle must lie inside the holder. An erase part paints 0 (the mean pixel) and
                        has no boxes. The query itself carries pos_cls and min_visible and nothing of a part
      q["at"]           without parts: the query (row, crop, at, ...) is itself the only part
      boxes             a part's boxes are shifted and clamped to its window as for q["crop"], then moved by (dx, dy); with
                        min_visible = f > 0 a box stays only if (seen - hidden) >= f * full, hidden = the sum over the
                        LATER parts of the area of the box their rectangles cover (`composed_boxes_numpy`). An area two
                        later parts share counts twice. f = 0 applies no rule at all -- a box that later parts cover
                        entirely stays -- so composed queries should set min_visible.
    A composed query takes no ratio / need_crop / crop_start. One composed query makes the plan `composed`: its words end
    with the composed section and `EpisodeAssembler` runs the composed launches; the other queries of the batch come out
    with the bits they have in a plan without it. im_info carries part 0's im_scale (1 for an erase part).
    A key that is none of `QUERY_KEYS` (`PART_KEYS` in a part) is refused."""
    queries, supports = list(queries), list(supports)
    if queries and holder_hw is None:
        raise ValueError("plan_episode: holder_hw is needed to plan queries")
    qs = [_plan_query(pool, q, holder_hw, target_size) for q in queries]
    ss = []
    for sup in supports:
        if len(sup) not in (2, 3):
            raise ValueError("plan_episode: a support is (row, box) or (row, box, color), got %d entries" % len(sup))
        s = _plan_support(pool, sup[0], sup[1], target_size, support_size)
        s["color"] = _color("color", sup[2]) if len(sup) == 3 else None
        ss.append(s)
    composed = any("parts" in q for q in qs)
    # (in a composed plan the queries' colour maps and thresholds travel in the composed section)
    augmented = (not composed and any(q.get(k) is not None for q in queries for k in AUGMENT_KEYS)) or \
        any(s["color"] is not None for s in ss)
    words = _pack_plan(qs, ss, augmented)
    c_off, max_parts = None, 0
    if composed:
        words, c_off, max_parts = _pack_composed(words, qs)
    return EpisodePlan(words, qs, ss, None if holder_hw is None else (int(holder_hw[0]), int(holder_hw[1])),
                       _aug_offset(qs, ss) if augmented else None, c_off, max_parts)


def episode_boxes_numpy(boxes, order, im_scale, x_s, y_s, clamp_x, clamp_y, pos_cls, max_num_box, min_visible=0.0):
    """minibatch.py:52-54 + fs_loader.py:183-315 for one image, in numpy. boxes: float32 [n][5] unscaled; clamp_x / clamp_y:
    upper clamp limit of that axis, < 0 for none -> (fs_gt_boxes [max][5], num_boxes, all-class gt_boxes [max][5], its count).
    min_visible = f > 0 (not in the reference): with u the shifted row before the clamp and v after it, a box is also dropped
    unless (v2 - v0) * (v3 - v1) >= f * ((u2 - u0) * (u3 - u1)), all in float32."""
    src = np.asarray(boxes, dtype=np.float32).reshape(-1, 5)[np.asarray(order, dtype=np.int64).reshape(-1)]
    gt = np.empty((src.shape[0], 5), dtype=np.float32)
    gt[:, 0:4] = src[:, 0:4].astype(np.float64) * float(im_scale)  # the product in double, rounded by the assignment
    gt[:, 4] = src[:, 4]
    gt[:, 0:4:2] -= np.float32(x_s)  # :215-216, :251-252
    gt[:, 1:4:2] -= np.float32(y_s)
    u = gt[:, 0:4].copy()
    if clamp_x >= 0:
        gt[:, 0:4:2] = np.clip(gt[:, 0:4:2], np.float32(0), np.float32(clamp_x))  # :219-220, :254-255, :281
    if clamp_y >= 0:
        gt[:, 1:4:2] = np.clip(gt[:, 1:4:2], np.float32(0), np.float32(clamp_y))
    if min_visible > 0:  # in front of both compactions, beside the degenerate-box filter below
        full = (u[:, 2] - u[:, 0]) * (u[:, 3] - u[:, 1])
        seen = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
        gt = gt[seen >= np.float32(min_visible) * full]
    fs = gt[gt[:, 4] == pos_cls].copy()  # :286-291
    fs[:, 4] = 1.0
    out = []
    for g in (fs, gt):  # :294-315
        g = g[~((g[:, 0] == g[:, 2]) | (g[:, 1] == g[:, 3]))]
        n = min(g.shape[0], max_num_box)
        pad = np.zeros((max_num_box, 5), dtype=np.float32)
        pad[:n] = g[:n]
        out += [pad, n]
    return tuple(out)


def composed_boxes_numpy(parts, pos_cls, max_num_box, min_visible=0.0):
    """The box rule of a composed query (csrc/episode.hip: episode_boxes_composed_kernel) in numpy, every step one float32
    operation. parts: in painting order, dicts with boxes (float32 [n][5] unscaled; None for an erase part), order, im_scale,
    x_s, y_s (the window's start), h, w (its size), dy, dx (its destination) and optionally clamp_x, clamp_y (default
    w - 1, h - 1; < 0 for none). Per part, in its order: u = the double product rounded to float32, minus the window start;
    v = u clamped to the window; the output row t = v + (dx, dy, dx, dy). hidden = 0, then for each LATER part r in order
    hidden += max(min(t2, dx_r + w_r - 1) - max(t0, dx_r), 0) * max(min(t3, dy_r + h_r - 1) - max(t1, dy_r), 0): where
    later parts overlap each other the area counts twice (conservative, and the same in any restatement). A row stays
    unless v0 == v2 or v1 == v3 (on v: the translation could merge distinct values) and, with min_visible = f > 0, unless
    (seen - hidden) < f * full, seen and full as in `episode_boxes_numpy`. f = 0 applies no rule: a covered box stays.
    -> (fs_gt_boxes [max][5], num_boxes, all-class gt_boxes [max][5], its count), both lists in walk order"""
    f32 = np.float32
    rects = [(f32(p["dx"]), f32(p["dy"]), f32(p["dx"] + p["w"] - 1), f32(p["dy"] + p["h"] - 1)) for p in parts]
    kept = [np.zeros((0, 5), dtype=np.float32)]
    for k, p in enumerate(parts):
        order = np.asarray(p.get("order", ()), dtype=np.int64).reshape(-1)
        if p.get("boxes") is None or not len(order):
            continue
        src = np.asarray(p["boxes"], dtype=np.float32).reshape(-1, 5)[order]
        u = np.empty((src.shape[0], 4), dtype=np.float32)
        u[:] = src[:, 0:4].astype(np.float64) * float(p["im_scale"])  # the product in double, rounded by the assignment
        u[:, 0::2] -= f32(p["x_s"])
        u[:, 1::2] -= f32(p["y_s"])
        v = u.copy()
        clamp_x, clamp_y = p.get("clamp_x", p["w"] - 1), p.get("clamp_y", p["h"] - 1)
        if clamp_x >= 0:
            v[:, 0::2] = np.clip(v[:, 0::2], f32(0), f32(clamp_x))
        if clamp_y >= 0:
            v[:, 1::2] = np.clip(v[:, 1::2], f32(0), f32(clamp_y))
        t = np.empty((src.shape[0], 5), dtype=np.float32)
        t[:, 0:4:2] = v[:, 0::2] + f32(p["dx"])
        t[:, 1:4:2] = v[:, 1::2] + f32(p["dy"])
        t[:, 4] = src[:, 4]
        keep = ~((v[:, 0] == v[:, 2]) | (v[:, 1] == v[:, 3]))
        if min_visible > 0:
            hidden = np.zeros((src.shape[0],), dtype=np.float32)
            for x1, y1, x2, y2 in rects[k + 1:]:
                ox = np.maximum(np.minimum(t[:, 2], x2) - np.maximum(t[:, 0], x1), f32(0))
                oy = np.maximum(np.minimum(t[:, 3], y2) - np.maximum(t[:, 1], y1), f32(0))
                hidden = hidden + ox * oy
            full = (u[:, 2] - u[:, 0]) * (u[:, 3] - u[:, 1])
            seen = (v[:, 2] - v[:, 0]) * (v[:, 3] - v[:, 1])
            keep &= (seen - hidden) >= f32(min_visible) * full
        kept.append(t[keep])
    gt = np.concatenate(kept, axis=0)
    fs = gt[gt[:, 4] == pos_cls].copy()
    fs[:, 4] = 1.0
    out = []
    for g in (fs, gt):
        n = min(g.shape[0], max_num_box)
        pad = np.zeros((max_num_box, 5), dtype=np.float32)
        pad[:n] = g[:n]
        out += [pad, n]
    return tuple(out)


class EpisodeAssembler:
    """`assemble(plan)`: one asynchronous plan upload and three launches fill `holders` (whose addresses never change: a
    ProgramTrainer recorded on holders.tensors() follows every later assemble) plus `all_cls_gt_boxes`, the loader's sixth
    return. Nothing here waits for the device except when a plan buffer comes round again while its batch is still queued:
    the buffers rotate behind an event each."""

    def __init__(self, pool, holders=None, pixel_means=None, support_size=None, n_buffers=2):
        if pool.device is None or not pool.frozen:
            raise RuntimeError("EpisodeAssembler: needs a frozen ImagePool on a device")
        self.pool, self.holders = pool, holders
        self.support_size = (holders.support_size if holders is not None else 320) if support_size is None else support_size
        means = np.asarray(cfg.PIXEL_MEANS if pixel_means is None else pixel_means, dtype=np.float32).reshape(-1)
        self._means = (ctypes.c_float * 3)(*[float(m) for m in means[:3]])  # kept alive: a recorded launch points at it
        self._means_p = ctypes.cast(self._means, ctypes.c_void_p)
        if holders is not None:
            self.all_cls_gt_boxes = torch.zeros_like(holders.gt_boxes)
            self.all_cls_num_boxes = torch.zeros_like(holders.num_boxes)
        self._ring = [[None, None, None] for _ in range(max(2, int(n_buffers)))]  # pinned words, device words, event
        self._next = 0

    def _upload(self, plan):
        """-> (device words, slot): the plan in the next buffer of the ring, copied on the current stream"""
        slot = self._ring[self._next % len(self._ring)]
        self._next += 1
        n = int(plan.words.size)
        if slot[2] is not None:
            slot[2].synchronize()  # the batch that read this buffer, n_buffers assembles ago
        if slot[0] is None or slot[0].numel() < n:
            slot[0] = torch.empty((max(2 * n, 1024),), dtype=torch.int32, pin_memory=True)
            slot[1] = torch.empty((slot[0].numel(),), dtype=torch.int32, device=self.pool.device)
        slot[0][:n].numpy()[...] = plan.words
        slot[1][:n].copy_(slot[0][:n], non_blocking=True)
        return slot[1], slot

    @staticmethod
    def _done(slot):
        if slot[2] is None:
            slot[2] = torch.cuda.Event()
        slot[2].record()

    def _supports(self, d_plan, plan, out):
        p = self.pool
        if plan.augmented:  # the supports' augmentation records follow the queries'
            lib().call("dana_episode_supports_aug", _p(p.data), p.data.numel(), _p(p.d_offsets), _p(p.d_meta), len(p),
                       _p(d_plan), int(plan.words.size), plan.s_off, plan.a_off + plan.batch * EP_AWORDS, plan.n_supports,
                       self._means_p, self.support_size, _p(out), _stream())
            return
        lib().call("dana_episode_supports", _p(p.data), p.data.numel(), _p(p.d_offsets), _p(p.d_meta), len(p), _p(d_plan),
                   int(plan.words.size), plan.s_off, plan.n_supports, self._means_p, self.support_size, _p(out), _stream())

    def assemble(self, plan):
        h, p = self.holders, self.pool
        if h is None:
            raise RuntimeError("EpisodeAssembler.assemble: built without holders")
        B, H, W = h.im_data.size(0), h.im_data.size(2), h.im_data.size(3)
        n_sup = B * h.support_ims.size(1)
        if plan.batch != B or plan.n_supports != n_sup or plan.holder_hw != (H, W):
            raise ValueError("EpisodeAssembler.assemble: the plan (%d queries, %d supports, holder %s) is not for these holders "
                             "(%d, %d, %s)" % (plan.batch, plan.n_supports, plan.holder_hw, B, n_sup, (H, W)))
        d_plan, slot = self._upload(plan)
        n_words, stream = int(plan.words.size), _stream()
        if plan.composed:  # still three launches; the supports' is the one it always was
            lib().call("dana_episode_queries_composed", _p(p.data), p.data.numel(), _p(p.d_offsets), _p(p.d_meta), len(p),
                       _p(d_plan), n_words, plan.c_off, plan.max_parts, B, self._means_p, _p(h.im_data), H, W,
                       _p(h.im_info), stream)
            if n_sup:
                self._supports(d_plan, plan, h.support_ims)
            lib().call("dana_episode_boxes_composed", _p(p.d_boxes), len(p.boxes), _p(p.d_meta), len(p), _p(d_plan), n_words,
                       plan.c_off, plan.max_parts, B, h.gt_boxes.size(1), _p(h.gt_boxes), _p(h.num_boxes),
                       _p(self.all_cls_gt_boxes), _p(self.all_cls_num_boxes), stream)
            self._done(slot)
            return h.tensors() + (self.all_cls_gt_boxes,)
        if plan.augmented:
            lib().call("dana_episode_queries_aug", _p(p.data), p.data.numel(), _p(p.d_offsets), _p(p.d_meta), len(p),
                       _p(d_plan), n_words, plan.q_off, plan.a_off, B, self._means_p, _p(h.im_data), H, W, _p(h.im_info),
                       stream)
        else:
            lib().call("dana_episode_queries", _p(p.data), p.data.numel(), _p(p.d_offsets), _p(p.d_meta), len(p), _p(d_plan),
                       n_words, plan.q_off, B, self._means_p, _p(h.im_data), H, W, _p(h.im_info), stream)
        if n_sup:
            self._supports(d_plan, plan, h.support_ims)
        if plan.augmented:
            lib().call("dana_episode_boxes_aug", _p(p.d_boxes), len(p.boxes), _p(p.d_meta), len(p), _p(d_plan), n_words,
                       plan.q_off, plan.a_off, B, h.gt_boxes.size(1), _p(h.gt_boxes), _p(h.num_boxes),
                       _p(self.all_cls_gt_boxes), _p(self.all_cls_num_boxes), stream)
        else:
            lib().call("dana_episode_boxes", _p(p.d_boxes), len(p.boxes), _p(p.d_meta), len(p), _p(d_plan), n_words,
                       plan.q_off, B, h.gt_boxes.size(1), _p(h.gt_boxes), _p(h.num_boxes), _p(self.all_cls_gt_boxes),
                       _p(self.all_cls_num_boxes), stream)
        self._done(slot)
        return h.tensors() + (self.all_cls_gt_boxes,)

    def support_crops(self, records, out=None):
        """records: a plan of supports only (`plan_episode(pool, (), supports)`) -> fp32 [N][3][S][S], what
        `encode_support_bank` / `encode_supports` (reshaped to [C][shot]) take"""
        if records.batch != 0 or records.n_supports < 1:
            raise ValueError("EpisodeAssembler.support_crops: need a plan of supports only")
        S = self.support_size
        if out is None:
            out = torch.empty((records.n_supports, 3, S, S), dtype=torch.float32, device=self.pool.device)
        _chk(out, "out")
        if out.numel() != records.n_supports * 3 * S * S:
            raise ValueError("EpisodeAssembler.support_crops: out must hold [%d][3][%d][%d]" % (records.n_supports, S, S))
        d_plan, slot = self._upload(records)
        self._supports(d_plan, records, out)
        self._done(slot)
        return out


# ---- views of pool frames: flip and multi-scale testing -------------------------------------------------------------------
# Test-time augmentation is not in the reference tree. A view is a query record of the format above -- the frame at its own
# scale, mirrored when the row is a flipped twin -- so `EpisodeAssembler.assemble` prepares the B * V view images with the
# kernels that exist; `postprocess.ensemble_views` maps their detections back and merges them.

class ViewSet:
    """What `postprocess.fold_views` needs to know about the views of a `plan_views` plan: `n_images`, `views` (per image),
    and `table`, host float32 [n_images * views][5] = (fw, fh, flip, area_lo, area_hi) per view in plan order -- the ORIGINAL
    frame's width and height, whether the view was mirrored, and its box-area window in original-image pixels^2.
    `scales` [n_images * views] are the views' im_scale, `rows` their pool rows."""

    columns = 5  # floats per table row

    def __init__(self, n_images, views, table, scales, rows):
        self.n_images, self.views = int(n_images), int(views)
        self.table = np.ascontiguousarray(table, dtype=np.float32).reshape(self.n_images * self.views, self.columns)
        self.scales, self.rows = np.asarray(scales, dtype=np.float64), np.asarray(rows, dtype=np.int64)
        self._dev = {}

    def table_dev(self, device):
        """the table on `device`, uploaded once and cached"""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.table if self.table.size else np.zeros((1, self.columns), np.float32)).to(device)
        return self._dev[device]


def _view_rows(pool, rows, flip):
    """-> per image (row, twin or None, h, w), checked"""
    out = []
    for entry in rows:
        if flip:
            if not isinstance(entry, (tuple, list)) or len(entry) != 2:
                raise ValueError("plan_views: flip=True needs (row, twin_row) per image, got %r" % (entry,))
            row, h, w = _pool_row(pool, entry[0])
            twin, _, _ = _pool_row(pool, entry[1])
            if pool.frame_of(twin) != pool.frame_of(row):
                raise ValueError("plan_views: row %d is no twin of row %d: they read different frames" % (twin, row))
            if int(pool.meta[twin, 2]) == int(pool.meta[row, 2]):
                raise ValueError("plan_views: row %d is no twin of row %d: both have flipped = %d (ImagePool.add_flipped "
                                 "makes the twin)" % (twin, row, int(pool.meta[row, 2])))
        else:
            if isinstance(entry, (tuple, list)):
                raise ValueError("plan_views: (row, twin_row) entries need flip=True, got %r" % (entry,))
            (row, h, w), twin = _pool_row(pool, entry), None
        out.append((row, twin, h, w))
    return out


def _view_size(h, w, scale):
    im_scale = float(scale) / float(min(h, w))  # blob.py:45, as _plan_query
    return im_scale, cv_round(h * im_scale), cv_round(w * im_scale)


def views_holder_hw(pool, rows, scales=(600,)):
    """(H, W) of the smallest holder that takes every view of `plan_views(pool, rows, scales)`: the maximum prepared size"""
    sizes = [_view_size(int(pool.meta[r, 0]), int(pool.meta[r, 1]), s)[1:]
             for e in rows for r in [_pool_row(pool, e[0] if isinstance(e, (tuple, list)) else e)[0]] for s in scales]
    return (max(s[0] for s in sizes), max(s[1] for s in sizes)) if sizes else (1, 1)


def scales_holder_hw(pool, rows, scales=(600,), ratios=None):
    """(H, W) of the smallest holder that takes every copy window `plan_episode` can make for these rows when a query draws
    its `target_size` from `scales` (multi-scale training). ratios: None, or one ratio per row (ratio_list_batch). Without
    ratios the bound is the maximum prepared size; with them it is `pad_plan`'s copy window of the uncropped image, which a
    ratio crop or a `crop` window only makes smaller."""
    rows = list(rows)
    ratios = [None] * len(rows) if ratios is None else [float(r) for r in ratios]
    if len(ratios) != len(rows):
        raise ValueError("scales_holder_hw: %d ratios for %d rows" % (len(ratios), len(rows)))
    H, W = 1, 1
    for entry, ratio in zip(rows, ratios):
        _, h, w = _pool_row(pool, entry)
        for s in scales:
            _, oh, ow = _view_size(h, w, s)
            if ratio is not None:
                oh, ow = pad_plan(oh, ow, ratio)[2:]
            H, W = max(H, oh), max(W, ow)
    return H, W


def plan_views(pool, rows, scales=(600,), flip=False, area_ranges=None, holder_hw=None):
    """Host only. The views of flip / multi-scale testing as one plan of query records. rows: one entry per image -- a pool
    row, or with flip=True (row, twin_row), the twin made by `ImagePool.add_flipped`. Image i's V = len(scales) * F views
    (F = 2 with flip, else 1) are records i * V + v, v = s * F + f: scale s, f = 0 the row as stored, f = 1 its twin. Every
    view is the whole frame prepared so that its SHORTER side is scales[s] (Q_SCALE = scales[s] / min(h, w), as `_plan_query`
    for that target_size), at the holder's top-left corner, with no crop, no clamp and no boxes. holder_hw defaults to
    `views_holder_hw`: every view of a batch lies in a holder of the largest view's size.
    area_ranges: None, or one (lo, hi) per scale: only boxes with lo <= area < hi in ORIGINAL-image pixels^2 are taken from
    that scale's views (upscaled views answer for small objects, downscaled ones for large; Detectron's
    BBOX_AUG.AREA_TH_LO / AREA_TH_HI, not in the reference). No default window is invented: None keeps everything.
    -> (EpisodePlan for query-only holders of n_images * V rows, ViewSet)"""
    scales = [float(_host_only("scales", s)) for s in scales]
    if not scales or not all(s > 0 for s in scales):
        raise ValueError("plan_views: scales must be positive, got %r" % (scales,))
    if area_ranges is None:
        area_ranges = [(-np.inf, np.inf)] * len(scales)
    area_ranges = [(float(lo), float(hi)) for lo, hi in area_ranges]
    if len(area_ranges) != len(scales):
        raise ValueError("plan_views: %d area ranges for %d scales" % (len(area_ranges), len(scales)))
    F = 2 if flip else 1
    images = _view_rows(pool, list(rows), bool(flip))
    if holder_hw is None:
        holder_hw = views_holder_hw(pool, [im[0] for im in images], scales)
    holder_hw = (int(holder_hw[0]), int(holder_hw[1]))
    qs, table = [], []
    for row, twin, h, w in images:
        for s, (scale, (lo, hi)) in enumerate(zip(scales, area_ranges)):
            im_scale, oh, ow = _view_size(h, w, scale)
            if oh > holder_hw[0] or ow > holder_hw[1]:
                raise ValueError("plan_episode: copy window %d x %d of row %d is larger than the holder (%d x %d)"
                                 % (oh, ow, row, holder_hw[0], holder_hw[1]))
            for f in range(F):
                r = twin if f else row
                qs.append(dict(row=r, im_scale=im_scale, oh=oh, ow=ow, y_s=0, x_s=0, copy_h=oh, copy_w=ow, out_h=oh, out_w=ow,
                               clamp_x=-1, clamp_y=-1, pos_cls=0, order=np.zeros((0,), dtype=np.int32), view=s * F + f))
                # a view is mirrored relative to the ORIGINAL image when its row's flipped bit says so
                table.append((float(w), float(h), float(int(pool.meta[r, 2])), lo, hi))
    plan = EpisodePlan(_pack_plan(qs, []), qs, [], holder_hw)
    views = ViewSet(len(images), len(scales) * F, np.asarray(table, dtype=np.float32).reshape(-1, 5),
                    [q["im_scale"] for q in qs], [q["row"] for q in qs])
    return plan, views


# ---- tiles of pool frames: tiled inference --------------------------------------------------------------------------------
# Every view above is the whole frame, so a small object in a large frame reaches the trunk as a cell or two. A tile is a
# query record whose copy window (Q_YS, Q_XS, Q_COPY_H, Q_COPY_W) is a part of the frame prepared at a LARGER scale:
# `episode_queries` samples the prepared frame at (x_s + x, y_s + y), so a tile image is bit-equal to that crop of the
# prepared full frame and needs no kernel of its own. `postprocess.ensemble_views` maps the tiles' boxes back (clip to the
# tile, seam rule, translate) and merges them with an optional full-frame view. Not in the reference tree.

class TileSet(ViewSet):
    """The `ViewSet` of a `plan_tiles` plan, which `postprocess.fold_tiles` / `ensemble_views` read. `table` is host float32
    [n_images * views][13] per view in plan order, everything in ORIGINAL-image pixels:
      0..4   fw, fh, flip, area_lo, area_hi   as a ViewSet's: the original frame, the row's flipped bit, the area window
      5, 6   x_off, y_off                     float32(x_s / im_scale), float32(y_s / im_scale): divided in float64, rounded once
      7, 8   tw, th                           float32(copy_w / im_scale), float32(copy_h / im_scale)
      9..12  lim_x1, lim_y1, lim_x2, lim_y2   in tile coordinates: float32(margin / im_scale) and float32((copy - 1 - margin) /
                                              im_scale) on an interior side, -inf / +inf on a side that is a side of the frame
    For a mirrored view (flip = 1) the offsets are those of its window in the MIRRORED frame; the fold un-mirrors after
    translating. The full-frame view has offsets 0, (tw, th) = (fw, fh) and infinite limits. `windows` is host int32
    [n_images * views][4] = (y_s, x_s, copy_h, copy_w) in prepared pixels of the view."""
    columns = 13

    def __init__(self, n_images, views, table, scales, rows, windows):
        super().__init__(n_images, views, table, scales, rows)
        self.windows = np.ascontiguousarray(windows, dtype=np.int32).reshape(self.n_images * self.views, 4)


def tile_windows(length, n, overlap=64, margin=4):
    """The windows of `n` tiles along an axis of `length` prepared pixels -> (starts [n], size): for n = 1 the whole axis,
    otherwise size = ceil((length + (n - 1) * overlap) / n) and start k = (k * (length - size)) // (n - 1). The first window
    starts at 0, the last ends at `length`, neighbours overlap by at least `overlap`.
    Coverage guarantee: every integer interval [a, b] of the axis with b - a <= overlap - 2 * margin lies in at least one
    window [s, s + size) in which it keeps `margin` from every INTERIOR side (a side that is not an end of the axis):
    a >= s + margin unless s = 0, and b <= s + size - 1 - margin unless s + size = length. (Take the first window whose far
    side lets the interval pass: it failed the previous one by b >= e - margin, neighbours share at least `overlap` pixels,
    so a >= b - (overlap - 2 * margin) >= e - overlap + margin >= s + margin.) ValueError for windows that cannot be:
    size > length; length - size < n - 1 (a grid so fine that two windows would coincide); overlap - 2 * margin < 1."""
    L, n, o, m = int(length), int(n), int(overlap), int(margin)
    if n < 1 or o < 0 or m < 0:
        raise ValueError("plan_tiles: need tiles >= 1, overlap >= 0, margin >= 0, got %d, %d, %d" % (n, o, m))
    if n == 1:
        return [0], L
    if o - 2 * m < 1:
        raise ValueError("plan_tiles: overlap %d - 2 * margin %d < 1: no box is safe from both of two neighbouring tiles' seams"
                         % (o, m))
    T = -(-(L + (n - 1) * o) // n)
    if T > L:
        raise ValueError("plan_tiles: %d tiles with overlap %d need windows of %d on an axis of %d prepared pixels" % (n, o, T, L))
    if L - T < n - 1:
        raise ValueError("plan_tiles: %d tiles of %d on an axis of %d prepared pixels would coincide (overlap %d)" % (n, T, L, o))
    return [(k * (L - T)) // (n - 1) for k in range(n)], T


def _tile_grid(grid):
    ny, nx = (int(_host_only("grid", g)) for g in grid)
    if ny < 1 or nx < 1:
        raise ValueError("plan_tiles: grid must be (ny >= 1, nx >= 1), got %r" % (tuple(grid),))
    return ny, nx


def _tile_sizes(h, w, grid, scale, overlap, margin, full_frame):
    """-> the (oh, ow) of every view of an h x w frame: the full frame first when there is one, then the tile size"""
    _, oh, ow = _view_size(h, w, scale)
    sizes = [(tile_windows(oh, grid[0], overlap, margin)[1], tile_windows(ow, grid[1], overlap, margin)[1])]
    if full_frame is not None:
        sizes.insert(0, _view_size(h, w, full_frame)[1:])
    return sizes


def tiles_holder_hw(pool, rows, grid, scale=600, overlap=64, margin=4, full_frame=600):
    """(H, W) of the smallest holder that takes every view of `plan_tiles` with these arguments: the largest of the tiles
    and the full-frame views"""
    grid = _tile_grid(grid)
    sizes = [s for e in rows for r in [_pool_row(pool, e[0] if isinstance(e, (tuple, list)) else e)[0]]
             for s in _tile_sizes(int(pool.meta[r, 0]), int(pool.meta[r, 1]), grid, scale, overlap, margin, full_frame)]
    return (max(s[0] for s in sizes), max(s[1] for s in sizes)) if sizes else (1, 1)


def plan_tiles(pool, rows, grid, scale=600, overlap=64, margin=4, flip=False, full_frame=600, area_ranges=None, holder_hw=None):
    """Host only. Tiled inference as one plan of query records. rows and flip as in `plan_views`. Every frame is prepared so
    that its SHORTER side is `scale` -- the magnification of the whole frame: scale=1200 with a 2 x 2 grid gives tiles of
    about 600 + overlap -- and cut into grid = (ny, nx) windows per `tile_windows`, `overlap` and `margin` in prepared pixels
    of the tile views; with full_frame = a target size (None: no such view) the whole frame at that size comes first, as
    `plan_views` would plan it. Image i's V = T * F views (T = ny * nx + 1 with the full frame, F = 2 with flip) are records
    i * V + v, v = t * F + f: t = 0 the full frame when present, then the tiles row-major (ty * nx + tx); f = 1 the twin, whose
    windows are the same numbers in the mirrored frame. A tile record copies its window of the prepared frame to the holder's
    top-left corner, with no clamp and no boxes. The grid is the same for every image so that V is.
    area_ranges: None or (full_range, tile_range), each (lo, hi) in ORIGINAL-image pixels^2, the table's area columns as in
    `plan_views`: the full frame answers for large boxes, the tiles for small ones. No default window is invented.
    holder_hw defaults to `tiles_holder_hw`. The coverage guarantee of `tile_windows` holds per axis, in prepared pixels: an
    object no larger than overlap - 2 * margin is whole, and clear of the seams, in at least one tile; larger objects are the
    full-frame view's. ValueError (naming the value) for the windows `tile_windows` refuses and for a view larger than the
    holder. -> (EpisodePlan for query-only holders of n_images * V rows, TileSet)"""
    ny, nx = grid = _tile_grid(grid)
    scale = float(_host_only("scale", scale))
    if not scale > 0 or (full_frame is not None and not float(_host_only("full_frame", full_frame)) > 0):
        raise ValueError("plan_tiles: scale and full_frame must be positive, got %r and %r" % (scale, full_frame))
    inf = (-np.inf, np.inf)
    if area_ranges is None:
        area_ranges = (inf, inf)
    if len(area_ranges) != 2:
        raise ValueError("plan_tiles: area_ranges is (full_range, tile_range), got %d ranges" % len(area_ranges))
    full_range, tile_range = [(float(lo), float(hi)) for lo, hi in area_ranges]
    F = 2 if flip else 1
    images = _view_rows(pool, list(rows), bool(flip))
    if holder_hw is None:
        holder_hw = tiles_holder_hw(pool, [im[0] for im in images], grid, scale, overlap, margin, full_frame)
    holder_hw = (int(holder_hw[0]), int(holder_hw[1]))
    m = int(margin)
    qs, table = [], []

    def view(row, twin, h, w, im_scale, oh, ow, y_s, x_s, ch, cw, area, t, whole=False):
        if ch > holder_hw[0] or cw > holder_hw[1]:
            raise ValueError("plan_episode: copy window %d x %d of row %d is larger than the holder (%d x %d)"
                             % (ch, cw, row, holder_hw[0], holder_hw[1]))
        # an interior side keeps `margin` prepared pixels; a side of the frame has no seam
        lim = (m / im_scale if x_s > 0 else -np.inf, m / im_scale if y_s > 0 else -np.inf,
               (cw - 1 - m) / im_scale if x_s + cw < ow else np.inf, (ch - 1 - m) / im_scale if y_s + ch < oh else np.inf)
        for f in range(F):
            r = twin if f else row
            qs.append(dict(row=r, im_scale=im_scale, oh=oh, ow=ow, y_s=y_s, x_s=x_s, copy_h=ch, copy_w=cw, out_h=ch, out_w=cw,
                           clamp_x=-1, clamp_y=-1, pos_cls=0, order=np.zeros((0,), dtype=np.int32), view=t * F + f))
            # (the whole frame in its own pixels, not its prepared size divided back)
            size = (float(w), float(h)) if whole else (cw / im_scale, ch / im_scale)
            table.append((float(w), float(h), float(int(pool.meta[r, 2]))) + area + (x_s / im_scale, y_s / im_scale) + size + lim)

    for row, twin, h, w in images:
        t = 0
        if full_frame is not None:
            im_scale, oh, ow = _view_size(h, w, full_frame)
            view(row, twin, h, w, im_scale, oh, ow, 0, 0, oh, ow, full_range, t, whole=True)
            t += 1
        im_scale, oh, ow = _view_size(h, w, scale)
        ys, th = tile_windows(oh, ny, overlap, margin)
        xs, tw = tile_windows(ow, nx, overlap, margin)
        for y_s in ys:
            for x_s in xs:
                view(row, twin, h, w, im_scale, oh, ow, y_s, x_s, th, tw, tile_range, t)
                t += 1
    plan = EpisodePlan(_pack_plan(qs, []), qs, [], holder_hw)
    # (the tuples hold Python floats: the divisions above are float64 and the table rounds them once)
    tiles = TileSet(len(images), (ny * nx + (full_frame is not None)) * F, np.asarray(table, dtype=np.float64).astype(np.float32)
                    .reshape(-1, 13), [q["im_scale"] for q in qs], [q["row"] for q in qs],
                    [(q["y_s"], q["x_s"], q["copy_h"], q["copy_w"]) for q in qs])
    return plan, tiles
