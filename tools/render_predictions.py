"""The prediction figure of a synthetic episode, written out; or (--time) what its three kernels cost.

    python tools/render_predictions.py [--out DIR] [--batch 2 --height 192 --width 256 --shot 2]
        builds a seeded synthetic episode (`synthetic.episode_inputs`, test-profile weights), runs the eval forward,
        `postprocess.detections_by_class(..., with_layout=True)` and `render.prediction_sheet`, and writes one PNG per image:
        prediction_<b>.png, plus episode_<b>.png (`render.episode_sheet`: the ground-truth boxes and the first shot). No
        image library is involved. How to read the files: tools/README.md.

    python tools/render_predictions.py --time [--json result.json]
        N = 4 canvases of 600 x 1000, 100 detections per image with labels, 3 shots of 320 x 320: `to_rgb`, `draw_boxes`
        (also with zero boxes: the binning pass alone) and `sheet`, each the median of 50 calls timed with a pair of
        device events after 10 warm-up calls; a device-to-device copy of the canvas bytes in the same run; and the host
        route -- the same tensors copied to the host and the numpy restatements run there (median of 5, host clock).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dana_amd  # noqa: E402
from dana_amd import ops, postprocess, render, synthetic as S  # noqa: E402
from dana_amd._lib import lib  # noqa: E402


def write_sheets(a, dev):
    m = dana_amd.get_model("DAnA", pretrained=False, use_BA_block=True, way=1, shot=a.shot, classes=["fg", "bg"])
    m.load_state_dict(S.fill_state_dict(m.state_dict(), seed=11, profile="test"))
    m.to(dev).eval()
    im, info, gt, nb, sup = [t.to(dev) for t in S.episode_inputs(a.batch, 1, a.shot, a.height, a.width, seed=5)]
    with torch.no_grad():
        out = m(im, info, gt, nb, sup)
    dets = postprocess.detections_by_class(out[0], out[1], out[2], info, 1, thresh=a.thresh, with_layout=True)
    side = min(a.side, a.height)
    pred = render.prediction_sheet(im, info, dets, sup, thickness=a.thickness, side=side)
    epis = render.episode_sheet(im, gt, nb, sup, shot=a.shot, thickness=a.thickness, side=side)
    os.makedirs(a.out, exist_ok=True)
    for b in range(a.batch):
        render.write_png(os.path.join(a.out, "prediction_%d.png" % b), pred[b])
        render.write_png(os.path.join(a.out, "episode_%d.png" % b), epis[b])
    print("wrote %d prediction and %d episode sheets (%d x %d and %d x %d pixels, %s detections per image) to %s"
          % (a.batch, a.batch, pred.size(2), pred.size(1), epis.size(2), epis.size(1), dets.counts.tolist(), a.out))


def event_median(fn, reps=50, warm=10):
    """median over `reps` calls of the device time between two events around one call, in microseconds"""
    for _ in range(warm):
        fn()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    t = [e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs]
    return dict(median_us=float(np.median(t)), min_us=float(np.min(t)), p90_us=float(np.percentile(t, 90)))


def host_median(fn, reps=5):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)))


def time_kernels(a, dev):
    N, H, W, n_det, n_shot, hs = 4, 600, 1000, 100, 3, 320
    rng = np.random.RandomState(7)
    im = torch.from_numpy((rng.randn(N, 3, H, W) * 64).astype(np.float32)).to(dev)
    sup = torch.from_numpy((rng.randn(N, n_shot, 3, hs, hs) * 64).astype(np.float32)).to(dev)
    wh = rng.uniform(40, 400, size=(N * n_det, 2))
    xy = rng.uniform(0, 1, size=(N * n_det, 2)) * (np.array([W - 1.0, H - 1.0]) - wh)
    score = np.sort(rng.uniform(0.05, 1.0, size=(N, n_det)), 1)[:, ::-1].reshape(-1, 1)
    boxes_h = np.concatenate((xy, xy + wh, score), 1).astype(np.float32)
    counts = np.full(N, n_det, np.int32)
    layout_h = np.concatenate((counts, np.arange(N + 1, dtype=np.int32) * n_det)).astype(np.int32)
    empty_h = np.concatenate((np.zeros(N, np.int32), layout_h[N:])).astype(np.int32)
    boxes, layout, empty = torch.from_numpy(boxes_h).to(dev), torch.from_numpy(layout_h).to(dev), torch.from_numpy(empty_h).to(dev)
    canvas = render.to_rgb(im)
    sup_rgb = render.to_rgb(sup)
    work, spare = canvas.clone(), torch.empty_like(canvas)
    nbytes = canvas.numel()
    dev_t = dict(
        to_rgb=event_median(lambda: render.to_rgb(im)),
        draw_boxes=event_median(lambda: render.draw_boxes(work, boxes, layout, thickness=2, labels=True)),
        draw_boxes_no_labels=event_median(lambda: render.draw_boxes(work, boxes, layout, thickness=2)),
        draw_boxes_zero_boxes=event_median(lambda: render.draw_boxes(work, boxes, empty, thickness=2, labels=True)),
        sheet=event_median(lambda: render.sheet(canvas, sup_rgb)),
        copy_canvas_d2d=event_median(lambda: lib().call("dana_copy_d2d", spare.data_ptr(), canvas.data_ptr(), nbytes, ops._stream())))
    drawn = render.draw_boxes(canvas.clone(), boxes, layout, thickness=2, labels=True)
    touched = int((drawn != canvas).any(-1).sum())
    host_t = dict(
        to_rgb=host_median(lambda: render.to_rgb_numpy(im.cpu().numpy())),
        draw_boxes=host_median(lambda: render.boxes_numpy(canvas.cpu().numpy(), boxes.cpu().numpy(), layout=layout.cpu().numpy(),
                                                          thickness=2, labels=True)),
        sheet=host_median(lambda: render.sheet_numpy(canvas.cpu().numpy(), sup_rgb.cpu().numpy())),
        d2h_only=host_median(lambda: (im.cpu(), sup.cpu(), boxes.cpu(), layout.cpu())))
    same = bool(np.array_equal(drawn.cpu().numpy(), render.boxes_numpy(canvas.cpu().numpy(), boxes_h, layout=layout_h, thickness=2,
                                                                       labels=True)))
    res = dict(shape=dict(images=N, height=H, width=W, detections_per_image=n_det, shots=n_shot, shot_size=hs,
                          canvas_bytes=nbytes, pixels_changed_by_draw=touched, tiles=N * -(-H // render.TILE[0]) * -(-W // render.TILE[1])),
               device_us=dev_t, host_route_ms=host_t, draw_equals_restatement=same, device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="render_predictions_out")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--shot", type=int, default=2)
    ap.add_argument("--side", type=int, default=160, help="side of a support shot on the sheet (at most the height)")
    ap.add_argument("--thickness", type=int, default=2)
    ap.add_argument("--thresh", type=float, default=0.05, help="score threshold of detections_by_class")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool runs on the device only")
    dev = torch.device("cuda:0")
    if a.time:
        time_kernels(a, dev)
    else:
        write_sheets(a, dev)


if __name__ == "__main__":
    main()
