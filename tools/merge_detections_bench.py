"""Time one `postprocess.ensemble_shots` call against the composition that gives the same result without it: slice the
`ClassDetections` apart, and per output list torch.cat, torch.sort, `dana_amd._C.nms`, index (utils.py:192-199 as written).

Default shape: B = 4 images, C = 5 classes, S = 3 shots, R = 300 rois -> 60 input lists of up to 300 rows, 20 output lists
of up to 900. The inputs are seeded synthetic detection lists (jittered boxes around shared objects, pairwise distinct
scores, each list in descending score order); the two ways are checked to agree bit for bit before anything is timed.

Both ways are timed in the same process, alternating, each call bracketed by a device synchronise (host clock); the
rounds are split into blocks so that the block-to-block spread of the medians is reported next to them.

    python tools/merge_detections_bench.py [--out result.json]
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
from dana_amd import postprocess as PP  # noqa: E402
from dana_amd.config import cfg  # noqa: E402


def synthetic_sweep(B, C, S, R, dev, seed=3, w=1000.0, h=600.0):
    """-> ClassDetections of B images x (C*S) sets, set c*S + s; every list holds between R/2 and R rows"""
    rng = np.random.RandomState(seed)
    P = B * C * S
    counts = rng.randint(R // 2, R + 1, P).astype(np.int32)
    total = int(counts.sum())
    score = ((rng.permutation(total) + 1.0) / (total + 1.0)).astype(np.float32)
    rows, at = [], 0
    for b in range(B):
        for c in range(C):
            n_obj = 12
            ctr = rng.uniform([60, 60], [w - 60, h - 60], size=(n_obj, 2))
            size = rng.uniform(40, 260, size=(n_obj, 2))
            for s in range(S):
                k = int(counts[(b * C + c) * S + s])
                o = rng.randint(0, n_obj, k)
                cxy = ctr[o] + rng.normal(0, 10, size=(k, 2))
                wh = size[o] * rng.uniform(0.7, 1.4, size=(k, 2))
                d = np.concatenate((cxy - wh / 2, cxy + wh / 2, score[at:at + k, None]), 1).astype(np.float32)
                rows.append(d[np.argsort(-d[:, 4], kind="stable")])
                at += k
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    packed = torch.from_numpy(np.concatenate(rows, 0)).to(dev)
    flat = [packed[int(offsets[p]):int(offsets[p + 1])] for p in range(P)]
    cd = PP.ClassDetections([flat[b * C * S:(b + 1) * C * S] for b in range(B)])
    cd.packed, cd.counts, cd.offsets, cd.num_classes = packed, torch.from_numpy(counts), torch.from_numpy(offsets), C * S
    cd.layout_dev = torch.from_numpy(np.concatenate((counts, offsets))).to(dev)
    return cd


def composition(cd, shots):
    """the only way to the same result without merge_detections: per output list, the chain of utils.py:192-199"""
    out = []
    for per_image in cd:
        row = []
        for c in range(len(per_image) // shots):
            final_dets = torch.cat(per_image[c * shots:(c + 1) * shots], 0)
            _, order = torch.sort(final_dets[:, 4], 0, True)
            final_dets = final_dets[order]
            keep = dana_amd._C.nms(final_dets[:, :4].contiguous(), final_dets[:, 4].contiguous(), cfg.TEST.NMS)
            row.append(final_dets[keep.view(-1).long()])
        out.append(row)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--shots", type=int, default=3)
    ap.add_argument("--rois", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=40, help="alternating (fused, composition) pairs per block")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    dev = torch.device("cuda:0")
    cd = synthetic_sweep(a.images, a.classes, a.shots, a.rois, dev)
    fused = lambda: PP.ensemble_shots(cd, a.shots)  # noqa: E731
    comp = lambda: composition(cd, a.shots)  # noqa: E731
    ens, ref = fused(), comp()
    same = all(torch.equal(x, y) for rx, ry in zip(ens, ref) for x, y in zip(rx, ry))
    kept = int(ens.total)
    for _ in range(10):  # warm both ways at the timed shape
        fused()
        comp()
    blocks = []
    for _ in range(a.blocks):
        tf, tc = [], []
        for _ in range(a.rounds):
            tf.append(timed(fused))
            tc.append(timed(comp))
        blocks.append(dict(fused_ms=float(np.median(tf)), composition_ms=float(np.median(tc)),
                           fused_min_ms=float(np.min(tf)), fused_p90_ms=float(np.percentile(tf, 90)),
                           composition_min_ms=float(np.min(tc)), composition_p90_ms=float(np.percentile(tc, 90))))
    mf = [b["fused_ms"] for b in blocks]
    mc = [b["composition_ms"] for b in blocks]
    res = dict(shape=dict(images=a.images, classes=a.classes, shots=a.shots, rois=a.rois, input_lists=len(cd.counts),
                          input_rows=int(cd.counts.sum()), output_lists=a.images * a.classes, output_rows=kept,
                          longest_concatenation=int(cd.counts.view(-1, a.shots).sum(1).max())),
               results_equal=bool(same), blocks=blocks, rounds_per_block=a.rounds,
               fused_ms=dict(median=float(np.median(mf)), lo=float(np.min(mf)), hi=float(np.max(mf))),
               composition_ms=dict(median=float(np.median(mc)), lo=float(np.min(mc)), hi=float(np.max(mc))),
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("the fused call and the composition disagree")


if __name__ == "__main__":
    main()
