"""Emit tests/golden/merge_dets.npz: a few seeded sets of per-shot detection lists with the REFERENCE's own answer for
their ensemble -- the literal chain of utils.py:192-199 (generate_pseudo_label): torch.cat of the lists,
`torch.sort(final_dets[:, 4], 0, True)`, `nms(boxes, scores, cfg.TEST.NMS)` with the reference's CPU operator (imported
through ref_import, which suppresses at IoU >= threshold, nms_cpu.cpp:60), then the index.

The file stores arrays only: per case the concatenated input rows, the per-shot counts and the rows the reference kept,
plus the threshold. Asserted, with the seed redrawn otherwise: scores pairwise distinct within a case (torch.sort's tie
order must not matter) and |IoU - threshold| >= 1e-4 for every suppression decision (the reference computes IoU in
float32, `postprocess.merge_numpy` in float64).

Run in the build container only:  python tests/golden/make_merge_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402
from dana_amd import postprocess as P  # noqa: E402

# (per-shot counts): an empty shot in the middle and a union that crosses one 64-bit mask word; two short lists; five shots
CASES = ((40, 0, 30), (5, 9), (23, 31, 17, 29, 26))


def draw(seed, counts, w=640.0, h=480.0):
    """every shot sees the same few objects: jittered boxes around shared centres, so that the NMS over the union has
    cross-shot suppression to do; each list in descending score order, as post-processing emits it"""
    rng = np.random.RandomState(seed)
    total = int(sum(counts))
    n_obj = max(total // 10, 2)
    ctr = rng.uniform([40, 40], [w - 40, h - 40], size=(n_obj, 2))
    size = rng.uniform(30, 160, size=(n_obj, 2))
    score = ((rng.permutation(total) + 1.0) / (total + 1.0)).astype(np.float32)  # pairwise distinct
    lists, at = [], 0
    for k in counts:
        o = rng.randint(0, n_obj, k)
        c = ctr[o] + rng.normal(0, 6, size=(k, 2))
        wh = size[o] * rng.uniform(0.8, 1.25, size=(k, 2))
        b = np.concatenate((c - wh / 2, c + wh / 2), 1)
        b[:, 0::2] = b[:, 0::2].clip(0, w - 1)
        b[:, 1::2] = b[:, 1::2].clip(0, h - 1)
        d = np.concatenate((b, score[at:at + k, None]), 1).astype(np.float32)
        lists.append(d[np.argsort(-d[:, 4], kind="stable")])
        at += k
    return lists


def reference_chain(nms, lists, thr):
    final_dets = None
    for cls_dets in lists:  # utils.py:188-195
        cls_dets = torch.from_numpy(cls_dets)
        final_dets = torch.cat((final_dets, cls_dets), 0) if final_dets is not None else cls_dets
    _, order = torch.sort(final_dets[:, 4], 0, True)
    final_dets = final_dets[order]
    keep = nms(final_dets[:, :4], final_dets[:, 4], thr)
    return final_dets[keep.view(-1).long()].numpy(), keep.view(-1).long().numpy()


def main():
    if not ref_import.available():
        raise SystemExit("the reference tree is not on this machine")
    ref = ref_import.load()
    thr = float(ref["cfg"].TEST.NMS)
    out = dict(nms_thresh=np.float64(thr), n_cases=np.int32(len(CASES)))
    for i, counts in enumerate(CASES):
        seed = 100 + 10 * i
        while True:
            lists = draw(seed, counts)
            mine = P.merge_numpy(lists, len(counts), thr, nms_inclusive=True)
            scores = np.concatenate([d[:, 4] for d in lists])
            if np.unique(scores).size == scores.size and mine["margin"] >= 1e-4:
                break
            seed += 1
        kept, keep = reference_chain(ref["C"].nms, lists, thr)
        assert 0 < len(kept) < len(scores), "the case must have something to suppress and something to keep"
        out["c%d_dets" % i] = np.concatenate(lists, 0)
        out["c%d_counts" % i] = np.asarray(counts, np.int32)
        out["c%d_out" % i] = kept
        out["c%d_keep" % i] = keep.astype(np.int32)
        out["c%d_seed" % i] = np.int32(seed)
        print("case %d: seed %d, %d rows -> %d kept, margin %.3e, merge_numpy %s" % (
            i, seed, len(scores), len(kept), mine["margin"], "agrees" if np.array_equal(mine["dets"][0], kept) else "DIFFERS"))
    path = os.path.join(HERE, "merge_dets.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
