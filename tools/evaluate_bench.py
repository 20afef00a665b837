"""Device evaluation (dana_amd/evaluate.py) at validation-set size: the device time of `DetectionEvaluator.compute()`
by HIP events, the bytes every kernel must move (from the shapes), and for comparison on the same box the host path
the code without the evaluator forces: a device-to-host copy of all detections plus the numpy restatement
(`evaluate.voc_numpy`), by default at a tenth of the images because it takes minutes at full size.

  python tools/evaluate_bench.py                       # 5 000 images x 20 classes x up to 100 detections, T = 1 and 10
  python tools/evaluate_bench.py --protocol coco       # the same data with some crowd objects, COCOeval's defaults
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/evaluate_bench.py --profile-run --thresholds 10

Prints one JSON line per configuration. Synthetic seeded data: per (class, image) 0..max-dets detections (60 % of them
jittered copies of that segment's boxes) and 0..3 ground-truth boxes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dana_amd import evaluate as E  # noqa: E402


def make(n_img, n_cls, max_dets, seed=0):
    rng = np.random.RandomState(seed)
    n_seg = n_img * n_cls
    per_g = rng.randint(0, 4, n_seg)
    g = int(per_g.sum())
    gseg = np.repeat(np.arange(n_seg), per_g)
    xy = rng.randint(0, 400, (g, 2))
    gt_box = np.concatenate((xy, xy + rng.randint(10, 150, (g, 2))), 1).astype(np.float32)
    gstart = np.concatenate(([0], np.cumsum(per_g)))
    per_d = rng.randint(0, max_dets + 1, n_seg)
    n = int(per_d.sum())
    dseg = np.repeat(np.arange(n_seg), per_d)
    xy = rng.uniform(0, 400, (n, 2))
    box = np.concatenate((xy, xy + rng.uniform(10, 150, (n, 2))), 1)
    has = (per_g[dseg] > 0) & (rng.rand(n) < 0.6)
    pick = gstart[dseg[has]] + (rng.rand(int(has.sum())) * per_g[dseg[has]]).astype(np.int64)
    box[has] = gt_box[pick] + rng.uniform(-8, 8, (int(has.sum()), 4))
    det = np.concatenate((box, rng.rand(n, 1)), 1).astype(np.float32)
    perm = rng.permutation(n)  # arrival order: mixed, as images come in
    return dict(det=det[perm], det_img=(dseg % n_img).astype(np.int32)[perm], det_cls=(dseg // n_img).astype(np.int32)[perm],
                gt_box=gt_box, gt_img=(gseg % n_img).astype(np.int32), gt_cls=(gseg // n_img).astype(np.int32),
                gt_difficult=(rng.rand(g) < 0.15).astype(np.uint8))


def kernel_bytes(n, g, n_seg, n_cls, T):
    """bytes each kernel of one dana_eval_ap must read + write at least once (algorithmic, from the shapes)"""
    bits = lambda v: max(int(v).bit_length(), 1)
    passes = lambda b: (b + 7) // 8
    pair = 12  # 64-bit key + 32-bit value
    p_gt, p_det, p_seg = passes(bits(n_seg)), passes(32 + bits(n_cls)), passes(bits(n_seg))
    return {
        "rs_hist_kernel": (p_gt * g + (p_det + p_seg) * n) * 8,
        "rs_scatter_kernel": (p_gt * g + (p_det + p_seg) * n) * 2 * pair,
        "det_keys_kernel": n * (4 + 4 + 4 + pair),
        "det_seg_keys_kernel": n * (8 + 4 + 4 + pair),
        "gt_keys_kernel": g * (8 + pair),
        "gt_gather_kernel": g * (pair + 16 + 1 + 16 + 1),
        "seg_offsets_kernel": (g + n) * 8 + n * 8 + (2 * n_seg + n_cls) * 4,
        "match_kernel": n * (4 + 4 + 20) + g * 17 + 2 * n_seg * 8 + T * n,
        "curves_ap_kernel": T * n * (1 + 8 + 8),
    }


def fill(ev, d, n_img):
    ev.add_ground_truth_packed(d["gt_box"], d["gt_img"], d["gt_cls"], d["gt_difficult"], num_images=n_img)
    step = 1 << 18
    for lo in range(0, d["det"].shape[0], step):  # appended in pieces: the buffers grow by doubling
        ev.add_packed(d["det"][lo:lo + step], d["det_img"][lo:lo + step], d["det_cls"][lo:lo + step])


def timed(compute, warmup, iters):
    """-> (ms per call by HIP events [iters], the last result)"""
    for _ in range(warmup):
        res = compute()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        e0.record()
        res = compute()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return np.asarray(times), res


def coco_form(d, crowd_share=0.05, seed=7):
    """the ground truth of make() as COCO's: (x, y, w, h) with the reference's + 1 widths, some objects crowd"""
    b = d["gt_box"]
    bbox = np.stack((b[:, 0], b[:, 1], b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1), 1).astype(np.float32)
    crowd = (np.random.RandomState(seed).rand(b.shape[0]) < crowd_share).astype(np.uint8)
    return bbox, crowd


def fill_coco(ev, d, n_img):
    bbox, crowd = coco_form(d)
    ev.add_ground_truth_packed(bbox, d["gt_img"], d["gt_cls"], crowd, num_images=n_img)
    step = 1 << 18
    for lo in range(0, d["det"].shape[0], step):
        ev.add_packed(d["det"][lo:lo + step], d["det_img"][lo:lo + step], d["det_cls"][lo:lo + step])
    return bbox, crowd


def main_coco(a, dev):
    """COCOeval's default parameters (T = 10, R = 101, A = 4, M = 3) on the data of make()"""
    d = make(a.images, a.classes, a.max_dets)
    n, g = d["det"].shape[0], d["gt_box"].shape[0]
    ev = E.CocoEvaluator(a.classes, device=dev)
    fill_coco(ev, d, a.images)
    if a.profile_run:
        for _ in range(5):
            res = ev.compute()
        torch.cuda.synchronize()
        print(json.dumps({"profile_run": True, "protocol": "coco", "n": n, "g": g, "summary": res.summarize().cpu().tolist()}))
        return
    times, res = timed(ev.compute, a.warmup, a.iters)
    out = {"protocol": "coco", "images": a.images, "classes": a.classes, "detections": n, "ground_truth": g,
           "thresholds": 10, "area_ranges": 4, "max_dets": list(E.COCO_MAX_DETS),
           "compute_ms_median": float(np.median(times)), "compute_ms_min": float(times.min()),
           "compute_ms_p90": float(np.percentile(times, 90)), "iters": a.iters, "warmup": a.warmup,
           "workspace_MiB": E.lib().query("dana_eval_coco_workspace_bytes", n, g, a.images, a.classes, 10, 101, 4, 3) / 2 ** 20,
           "summary": dict(zip(E.COCO_SUMMARY_NAMES, [round(x, 6) for x in res.summarize().cpu().tolist()]))}
    # the nearest existing workload on the same data in the same process: the VOC compute() at T = 10
    voc = E.DetectionEvaluator(a.classes, E.COCO_THRESHOLDS, device=dev)
    fill(voc, d, a.images)
    vt, _ = timed(voc.compute, a.warmup, a.iters)
    out.update(voc_T10_compute_ms_median=float(np.median(vt)), coco_over_voc=float(np.median(times) / np.median(vt)),
               curve_work_factor_A_times_M=12)
    del voc
    if a.host_scale > 0:
        hi = max(int(a.images * a.host_scale), 1)
        ds = make(hi, a.classes, a.max_dets, seed=1)
        ev_small = E.CocoEvaluator(a.classes, device=dev)
        bbox, crowd = fill_coco(ev_small, ds, hi)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = ev_small._det[:ev_small.num_rows].cpu().numpy()  # what the code without the evaluator has to do
        img, cls = ev_small._img[:ev_small.num_rows].cpu().numpy(), ev_small._cls[:ev_small.num_rows].cpu().numpy()
        t1 = time.perf_counter()
        ref = E.coco_numpy(rows, img, cls, bbox, ds["gt_img"], ds["gt_cls"], hi, a.classes, crowd)
        t2 = time.perf_counter()
        got = ev_small.compute()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        st, _ = timed(ev_small.compute, 3, 10)
        diff = float(np.abs(got.summarize().cpu().numpy() - E.coco_summarize_numpy(ref["precision"], ref["recall"])).max())
        out.update(host_images=hi, host_detections=int(rows.shape[0]), host_d2h_s=t1 - t0, host_numpy_s=t2 - t1,
                   device_same_size_wall_s=t3 - t2, device_same_size_ms_median=float(np.median(st)),
                   host_vs_device_max_summary_diff=diff)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--protocol", choices=("voc", "coco"), default="voc")
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--max-dets", type=int, default=100)
    ap.add_argument("--thresholds", default="1,10")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--host-scale", type=float, default=0.1, help="share of the images the host path runs on (0: skip)")
    ap.add_argument("--profile-run", action="store_true", help="five compute() calls and nothing else (for rocprofv3)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    if a.protocol == "coco":
        return main_coco(a, dev)
    d = make(a.images, a.classes, a.max_dets)
    n, g = d["det"].shape[0], d["gt_box"].shape[0]
    for T in [int(x) for x in a.thresholds.split(",")]:
        thr = E.COCO_THRESHOLDS[:T] if T <= 10 else tuple(np.linspace(0.5, 0.95, T))
        ev = E.DetectionEvaluator(a.classes, thr, device=dev)
        fill(ev, d, a.images)
        if a.profile_run:
            for _ in range(5):
                res = ev.compute()
            torch.cuda.synchronize()
            print(json.dumps({"profile_run": True, "n": n, "g": g, "T": T, "mean_ap": res.mean_ap().cpu().tolist()}))
            continue
        for _ in range(a.warmup):
            res = ev.compute()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(a.iters):
            e0.record()
            res = ev.compute()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        times = np.asarray(times)
        out = {"images": a.images, "classes": a.classes, "detections": n, "ground_truth": g, "thresholds": T,
               "compute_ms_median": float(np.median(times)), "compute_ms_min": float(times.min()),
               "compute_ms_p90": float(np.percentile(times, 90)), "iters": a.iters, "warmup": a.warmup,
               "workspace_MiB": E.lib().query("dana_eval_ap_workspace_bytes", n, g, a.images, a.classes, T) / 2 ** 20,
               "kernel_bytes": kernel_bytes(n, g, a.images * a.classes, a.classes, T),
               "mean_ap": [round(x, 6) for x in res.mean_ap().cpu().tolist()]}
        if a.host_scale > 0:
            hi = max(int(a.images * a.host_scale), 1)
            ev_small = E.DetectionEvaluator(a.classes, thr, device=dev)
            ds = make(hi, a.classes, a.max_dets, seed=1)
            fill(ev_small, ds, hi)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = ev_small._det[:ev_small.num_rows].cpu().numpy()  # what the code without the evaluator has to do
            img, cls = ev_small._img[:ev_small.num_rows].cpu().numpy(), ev_small._cls[:ev_small.num_rows].cpu().numpy()
            t1 = time.perf_counter()
            ref = E.voc_numpy(rows, img, cls, ds["gt_box"], ds["gt_img"], ds["gt_cls"], ds["gt_difficult"], hi, a.classes,
                              np.asarray(thr))
            t2 = time.perf_counter()
            got = ev_small.compute()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            dev_ap = got.ap.cpu().numpy()
            out.update(host_images=hi, host_detections=int(rows.shape[0]), host_d2h_s=t1 - t0, host_numpy_s=t2 - t1,
                       device_same_size_wall_s=t3 - t2, host_vs_device_max_ap_diff=float(np.nanmax(np.abs(dev_ap - ref["ap"]))))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
