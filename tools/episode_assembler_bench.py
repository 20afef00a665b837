"""One batch of episodes at the reference's sizes (bs 4, way 2, shot 3; 375x500 and 480x333 sources at target 600, 320 x 320
supports, 600 x 600 holders: the batch of tests/test_gpu_episode_assembler.py::test_reference_sizes_feed_the_model), built
by the per-image path (prep_im_for_blob -> EpisodeHolders.put_*) and by EpisodeAssembler.assemble, in one process.

    python tools/episode_assembler_bench.py [--reps 200]

Both paths are warmed, then alternated `--reps` times each. Per path: GPU time per batch from device events around the
batch, host enqueue time per batch from a host clock with no synchronise inside the window (the device is drained between
windows), the C-ABI launches per batch (counted through the recorder hook) and the bytes each path moves, computed from the
shapes. The per-image path is timed twice: drawing its frames from the host each time (what a loader over EpisodeHolders
does) and with the uint8 frames already on the device (so that the difference is the kernels' and the launches', not the
upload's). Prints one JSON line. profiles/episode_assembler.md was made with it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MEANS = np.array([102.9801, 115.9465, 122.7717], dtype=np.float32)
SPECS = [(375, 500, [[30, 40, 200, 300, 1], [250, 100, 480, 360, 2], [9, 9, 18, 13, 1]]),
         (480, 333, [[20, 30, 300, 400, 2], [100, 200, 320, 470, 1]]),
         ("flip", 0, [[299, 40, 469, 300, 1], [19, 100, 249, 360, 2]]),
         (375, 500, [[60, 50, 400, 330, 1]])]
QUERIES = [dict(row=0, ratio=1.0, pos_cls=1, order=[2, 0, 1]), dict(row=1, ratio=1.0, pos_cls=2),
           dict(row=2, ratio=1.0, pos_cls=2, order=[1, 0]), dict(row=3, ratio=1.0, pos_cls=1)]
BOXES = [(0, (30, 40, 200, 300)), (1, (100, 200, 320, 470)), (2, (299, 40, 469, 300)), (3, (60, 50, 400, 330)),
         (0, (250, 100, 480, 360)), (1, (20, 30, 300, 400))]
B, WS, TARGET, S, H, W = 4, 6, 600, 320, 600, 600


class _Count:
    def __init__(self):
        self.n = 0

    def add_call(self, fn, name, args):
        self.n += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    from dana_amd import _lib, pipeline as PL
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(8)
    pool, src = PL.ImagePool(dev), []
    for spec in SPECS:
        if spec[0] == "flip":
            src.append((src[spec[1]][0], True))
            pool.add_flipped(spec[1], spec[2])
        else:
            src.append((rng.randint(0, 256, size=(spec[0], spec[1], 3)).astype(np.uint8), False))
            pool.add(src[-1][0], spec[2])
    pool.freeze()
    sups = [BOXES[(b + k) % 6] for b in range(B) for k in range(WS)]
    resident = [torch.from_numpy(im).to(dev) for im, _ in src]
    hold_ref = PL.EpisodeHolders(B, 2, 3, H, W, dev)
    hold_new = PL.EpisodeHolders(B, 2, 3, H, W, dev)
    asm = PL.EpisodeAssembler(pool, hold_new, pixel_means=MEANS)
    nb = hold_ref.gt_boxes.size(1)

    def per_image(from_host):
        """the loop a loader over EpisodeHolders runs: every drawn image is prepared whole, once per draw"""
        plan = PL.plan_episode(pool, QUERIES, sups, holder_hw=(H, W))  # (the same host decisions; cheap next to the rest)
        frame = (lambda r: torch.from_numpy(src[r][0]).to(dev)) if from_host else (lambda r: resident[r])
        for b, q in enumerate(plan.queries):
            im, s = PL.prep_im_for_blob(frame(q["row"]), MEANS, TARGET, flipped=src[q["row"]][1])
            hold_ref.put_query(b, im, s, q["y_s"], q["x_s"], q["copy_h"], q["copy_w"])
        for n, (row, box) in enumerate(sups):
            im, s = PL.prep_im_for_blob(frame(row), MEANS, TARGET, flipped=src[row][1])
            hold_ref.put_support(n // WS, n % WS, im, (np.array(box, dtype=np.float32) * s).astype(np.int16))
        fs, n_fs, _, _ = plan.boxes_numpy(pool, nb)
        for b in range(B):
            hold_ref.put_boxes(b, fs[b][:n_fs[b]])
        return plan

    def assemble():
        return asm.assemble(PL.plan_episode(pool, QUERIES, sups, holder_hw=(H, W)))

    paths = {"per_image_host_frames": lambda: per_image(True), "per_image_resident_frames": lambda: per_image(False),
             "assemble": assemble}
    launches = {}
    for name, fn in paths.items():  # warm-up, the launch counts, and the two paths agree
        fn()
        _lib.RECORDER = rec = _Count()
        try:
            fn()
        finally:
            _lib.RECORDER = None
        launches[name] = rec.n
    torch.cuda.synchronize()
    for a, b in zip(hold_ref.tensors(), hold_new.tensors()):
        assert torch.equal(a, b), "the two paths differ"
    gpu, host = {k: [] for k in paths}, {k: [] for k in paths}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.reps):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            fn()
            host[name].append((time.perf_counter() - t0) * 1e3)
            e1.record()
            e1.synchronize()
            gpu[name].append(e0.elapsed_time(e1))
    # bytes from shapes: per-image = every drawn frame read, its whole prepared fp32 image written, the crop read back,
    # the holder slice written; assemble = the distinct frames read once (upper bound: taps are cached), the holders written
    plan = PL.plan_episode(pool, QUERIES, sups, holder_hw=(H, W))
    draws = plan.queries + plan.supports
    frame_b = sum(int(pool.meta[d["row"], 0]) * int(pool.meta[d["row"], 1]) * 3 for d in draws)
    prepared_b = sum(d["oh"] * d["ow"] * 12 for d in draws)
    crops_b = sum(q["copy_h"] * q["copy_w"] * 12 for q in plan.queries) + sum(s["cw"] * s["ch"] * 12 for s in plan.supports)
    holders_b = B * 3 * H * W * 4 + B * WS * 3 * S * S * 4
    small_b = B * 12 + B * nb * 20 * 2 + B * 8 * 2
    moved = {"per_image_host_frames": {"h2d": frame_b + B * 12 + int(sum(plan.boxes_numpy(pool, nb)[1])) * 20,
                                       "device_read": frame_b + crops_b, "device_written": prepared_b + holders_b + small_b},
             "per_image_resident_frames": {"h2d": B * 12 + int(sum(plan.boxes_numpy(pool, nb)[1])) * 20,
                                           "device_read": frame_b + crops_b, "device_written": prepared_b + holders_b + small_b},
             "assemble": {"h2d": int(plan.words.nbytes), "device_read": pool.nbytes + int(plan.words.nbytes),
                          "device_written": holders_b + small_b}}
    # host-to-device copies per batch: frames, one im_info row per query, one box block per query with boxes | the plan
    with_boxes = int((plan.boxes_numpy(pool, nb)[1] > 0).sum())
    for name, n in (("per_image_host_frames", len(draws) + B + with_boxes), ("per_image_resident_frames", B + with_boxes),
                    ("assemble", 1)):
        moved[name]["h2d_copies"] = n
    out = {"label": args.label, "reps": args.reps, "shape": "B %d, way 2, shot 3, holders %dx%d, supports %d" % (B, H, W, S),
           "pool_bytes": pool.nbytes, "plan_bytes": int(plan.words.nbytes)}
    for name in paths:
        g, h = np.array(gpu[name]), np.array(host[name])
        out[name] = {"gpu_ms_median": round(float(np.median(g)), 4), "gpu_ms_min": round(float(g.min()), 4),
                     "host_ms_median": round(float(np.median(h)), 4), "host_ms_min": round(float(h.min()), 4),
                     "c_abi_launches": launches[name], "bytes": moved[name]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
