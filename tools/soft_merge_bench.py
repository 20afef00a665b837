"""Time one `postprocess.ensemble_shots` call under each suppression method ("hard", "linear", "gaussian"), with and
without box voting, at the shot-ensemble shape of tools/merge_detections_bench.py (B = 4 images, C = 5 classes, S = 3 shots,
R = 300 rois: 60 seeded input lists, 20 output lists of up to 900 rows), and beside them what the soft forms replace:
reading the lists back and looping on the host (`postprocess.merge_soft_numpy`, method "linear", the vectorised one).

Per form two figures: the host clock around one call bracketed by device synchronises (the whole call: Python, the
workspace, the launches, the D2H read of the layout), and device events recorded around the same call (the stretch of the
stream the call occupies; with six launches or fewer it is the kernels plus the gaps the host leaves between them). The
forms alternate inside a round; rounds are split into blocks and the spread of the block medians is reported.

    python tools/soft_merge_bench.py [--out result.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from merge_detections_bench import synthetic_sweep  # noqa: E402
from dana_amd import postprocess as PP  # noqa: E402
from dana_amd.config import cfg  # noqa: E402

VOTE = 0.8


def timed(fn):
    """-> (host ms around the call with a synchronise on both sides, device-event ms around the same call)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--shots", type=int, default=3)
    ap.add_argument("--rois", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=40, help="rounds per block; a round runs every form once")
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    dev = torch.device("cuda:0")
    cd = synthetic_sweep(a.images, a.classes, a.shots, a.rois, dev)
    forms = {}
    for method in ("hard", "linear", "gaussian"):
        for vote in (False, True):
            kw = dict(method=method, vote_thresh=VOTE if vote else None)
            forms[method + ("+vote" if vote else "")] = (lambda kw=kw: PP.ensemble_shots(cd, a.shots, **kw))
    emitted = {}
    for name, fn in forms.items():  # warm every form at the timed shape
        for _ in range(10):
            m = fn()
        emitted[name] = dict(total=int(m.total), longest=int(m.counts.max()))
    # the linear form agrees with the host restatement, bit for bit, before anything is timed
    lists = [d.cpu().numpy() for per_image in cd for d in per_image]
    t0 = time.perf_counter()
    ref = PP.merge_soft_numpy(lists, a.shots, cfg.TEST.NMS, method="linear", vote_thresh=VOTE)
    m = forms["linear+vote"]()
    got, exp = m.packed[:m.total].cpu().numpy(), np.concatenate(ref["dets"], 0)
    same = got.shape == exp.shape and bool(np.array_equal(got.view(np.int32), exp.view(np.int32)))
    host_ms = []
    for _ in range(a.host_repeats):  # read the lists back, loop on the host (no voting)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        back = [d.cpu().numpy() for per_image in cd for d in per_image]
        PP.merge_soft_numpy(back, a.shots, cfg.TEST.NMS, method="linear")
        host_ms.append((time.perf_counter() - t0) * 1e3)
    blocks = []
    for _ in range(a.blocks):
        t = {name: ([], []) for name in forms}
        for _ in range(a.rounds):
            for name, fn in forms.items():
                h, d = timed(fn)
                t[name][0].append(h)
                t[name][1].append(d)
        blocks.append({name: dict(host_ms=float(np.median(h)), device_ms=float(np.median(d)), host_min_ms=float(np.min(h)),
                                  host_p90_ms=float(np.percentile(h, 90))) for name, (h, d) in t.items()})
    summary = {}
    for name in forms:
        hs, ds = [b[name]["host_ms"] for b in blocks], [b[name]["device_ms"] for b in blocks]
        summary[name] = dict(host_ms=dict(median=float(np.median(hs)), lo=float(np.min(hs)), hi=float(np.max(hs))),
                             device_ms=dict(median=float(np.median(ds)), lo=float(np.min(ds)), hi=float(np.max(ds))),
                             emitted_rows=emitted[name]["total"], longest_output_list=emitted[name]["longest"])
    res = dict(shape=dict(images=a.images, classes=a.classes, shots=a.shots, rois=a.rois, input_lists=len(cd.counts),
                          input_rows=int(cd.counts.sum()), output_lists=a.images * a.classes,
                          longest_concatenation=int(cd.counts.view(-1, a.shots).sum(1).max())),
               linear_vote_equals_restatement=same, forms=summary, blocks=blocks, rounds_per_block=a.rounds,
               host_readback_and_numpy_linear_ms=host_ms, vote_thresh=VOTE, device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("the device and the host restatement disagree")


if __name__ == "__main__":
    main()
