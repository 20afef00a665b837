"""Error diagnosis (dana_amd/diagnose.py `DetectionDiagnoser`) at validation-set size: the device time of `compute()` by HIP
events, against two baselines on the same box and the same data: `DetectionEvaluator.compute()` at one threshold (what the
diagnosis costs on top of the AP it starts from), and the host route the code without it forces -- a device-to-host copy
of every list plus the numpy restatement (`diagnose.tide_numpy`), by default at a tenth of the images -- whose results are
compared with the device's at that size.

  python tools/diagnose_bench.py                  # 5 000 images x 20 classes x up to 100 detections
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/diagnose_bench.py --profile-run

Prints one JSON line. Synthetic seeded data: 1..7 objects per image with random classes; the list of (image, class) holds
20..100 rows, each a jittered copy of one of the image's objects (with probability 0.5 when the object has the list's
class, 0.25 when not: a class sweep claims other classes' objects) or a random box; near-copies score higher.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dana_amd import diagnose as D, evaluate as E  # noqa: E402


def make(n_img, n_cls, n_det, dev, seed=0):
    """-> (det [n,5], det_img [n], det_cls [n] on the device, gt_box, gt_img, gt_cls on the host)"""
    rs = np.random.RandomState(seed)
    per = rs.randint(1, 8, n_img)
    g = int(per.sum())
    gt_img = np.repeat(np.arange(n_img), per).astype(np.int32)
    gt_cls = rs.randint(0, n_cls, g).astype(np.int32)
    xy = rs.uniform(0, 600, (g, 2))
    gt_box = np.concatenate((xy, xy + rs.uniform(20, 300, (g, 2))), 1).astype(np.float32)
    first = np.concatenate(([0], np.cumsum(per)[:-1]))
    gen = torch.Generator(device=dev).manual_seed(seed)
    shape = (n_img, n_cls, n_det)
    u = lambda *s: torch.rand(*s, generator=gen, device=dev)
    pick = torch.from_numpy(first).to(dev).view(-1, 1, 1) + (u(*shape) * torch.from_numpy(per).to(dev).view(-1, 1, 1)).long()
    obj = torch.from_numpy(gt_box).to(dev)[pick]
    own = torch.from_numpy(gt_cls).to(dev)[pick] == torch.arange(n_cls, device=dev).view(1, -1, 1)
    near = u(*shape) < torch.where(own, 0.5, 0.25)
    jitter = (u(*shape, 4) - 0.5) * 0.5 * (obj[..., 2:] - obj[..., :2]).repeat(1, 1, 1, 2) * u(*shape, 1)
    xy = u(*shape, 2) * 600
    rand = torch.cat((xy, xy + 20 + u(*shape, 2) * 280), -1)
    box = torch.where(near.unsqueeze(-1), obj + jitter, rand)
    score = torch.where(near, 0.3 + 0.7 * u(*shape), 0.6 * u(*shape))
    keep = torch.arange(n_det, device=dev).view(1, 1, -1) < (20 + (u(n_img, n_cls, 1) * (n_det - 19)).long()).clamp(max=n_det)
    det = torch.cat((box, score.unsqueeze(-1)), -1).float()[keep].contiguous()
    img = torch.arange(n_img, device=dev, dtype=torch.int32).view(-1, 1, 1).expand(shape)[keep].contiguous()
    cls = torch.arange(n_cls, device=dev, dtype=torch.int32).view(1, -1, 1).expand(shape)[keep].contiguous()
    return det, img, cls, gt_box, gt_img, gt_cls


def fill(ev, data, n_img):
    det, img, cls, gt_box, gt_img, gt_cls = data
    ev.add_ground_truth_packed(gt_box, gt_img, gt_cls, num_images=n_img)
    ev.add_packed(det, img, cls, num_images=n_img)
    return ev


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


def no_nan(x):
    if isinstance(x, dict):
        return {k: no_nan(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [no_nan(v) for v in x]
    return None if isinstance(x, float) and x != x else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--detections", type=int, default=100, help="the longest list of one (image, class)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-scale", type=float, default=0.1, help="share of the images the host route runs on (0: skip)")
    ap.add_argument("--profile-run", action="store_true", help="five compute() calls and nothing else (for rocprofv3)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diagnose_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    data = make(a.images, a.classes, a.detections, dev)
    dg = fill(D.DetectionDiagnoser(a.classes, device=dev), data, a.images)
    if a.profile_run:
        for _ in range(5):
            res = dg.compute()
        torch.cuda.synchronize()
        print(json.dumps(no_nan({"profile_run": True, "rows": dg.num_rows, "summary": res.summary()["count"]})))
        return
    times, res = timed(dg.compute, a.warmup, a.iters)
    ev = fill(E.DetectionEvaluator(a.classes, (0.5,), device=dev), data, a.images)
    etimes, eres = timed(ev.compute, a.warmup, a.iters)
    s = res.summary()
    out = dict(images=a.images, classes=a.classes, rows=dg.num_rows, ground_truth=int(data[3].shape[0]),
               compute_ms_median=float(np.median(times)), compute_ms_min=float(times.min()),
               compute_ms_p90=float(np.percentile(times, 90)), iters=a.iters, warmup=a.warmup,
               evaluator_ms_median=float(np.median(etimes)), evaluator_ms_min=float(etimes.min()),
               baseline_ap_equals_evaluator=bool(torch.equal(res.ap.view(torch.int64), eres.ap[:, 0].contiguous().view(torch.int64))),
               workspace_MiB=D.lib().query("dana_diagnose_errors_workspace_bytes", dg.num_rows, int(data[3].shape[0]),
                                           a.images, a.classes) / 2 ** 20,
               mean_ap=s["mean_ap"], count=s["count"], delta_map={k: round(v, 6) for k, v in s["delta_map"].items()})
    if a.host_scale > 0:
        hi = max(int(a.images * a.host_scale), 1)
        small = make(hi, a.classes, a.detections, dev, seed=1)
        dg_small = fill(D.DetectionDiagnoser(a.classes, device=dev), small, hi)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det, img, cls = [x.cpu().numpy() for x in small[:3]]  # what the code without the diagnoser has to do
        t1 = time.perf_counter()
        diff = np.zeros(small[3].shape[0], np.uint8)
        ref = D.tide_numpy(det, img, cls, small[3], small[4], small[5], diff, hi, a.classes)
        t2 = time.perf_counter()
        st, got = timed(dg_small.compute, 2, 5)
        valid = int(ref["cls_offsets"][-1])
        same = all(np.array_equal(getattr(got, k).cpu().numpy(), ref[k])
                   for k in ("cls_offsets", "tpfp", "npos", "det_type", "det_ref", "gt_state", "counts", "confusion"))
        same = same and np.array_equal(got.order.cpu().numpy()[:valid], ref["order"][:valid])
        fx, rf = got.ap_fixed.cpu().numpy(), ref["ap_fixed"]
        fin = np.isfinite(rf)
        out.update(host_images=hi, host_rows=int(det.shape[0]), host_d2h_s=t1 - t0, host_numpy_s=t2 - t1,
                   device_same_size_ms_median=float(np.median(st)), host_equals_device_integers=bool(same),
                   host_nan_pattern_equal=bool(np.array_equal(np.isnan(fx), np.isnan(rf))),
                   ap_fixed_max_rel_diff=float((np.abs(fx - rf)[fin] / np.maximum(np.abs(rf[fin]), 1e-300)).max()) if fin.any() else 0.,
                   host_min_iou_margin=D.diagnose_min_iou_margin(det, img, cls, small[3], small[4], small[5], hi, a.classes))
    print(json.dumps(no_nan(out)), flush=True)


if __name__ == "__main__":
    main()
