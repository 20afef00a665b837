"""What training-time augmentation costs in the episode assembler: one batch at bs 4, way 2, shot 3 into 600 x 1000 holders
(375x500, 333x500, 300x500 sources and a flipped twin at target 600: 600x800, 600x901, 600x1000; 24 supports of 320 x 320),
assembled by the plain launches and by the augmented ones with a colour map on every query and every support and a
visibility threshold on every query, in one process.

    python tools/episode_augment_bench.py [--reps 200] [--block 20]

Both paths are warmed and checked (identity maps through the augmented launches must give the plain bits), then timed in
alternating blocks of `--block` batches until each has `--reps`. Per path:
  gpu_ms     the interval between two device events around one batch (plan upload + three launches), device drained first
  host_ms    a host clock around the same calls, `plan_episode` included, no synchronise inside the window
  device_ms  the same interval with the batch enqueued behind a ~10 ms matrix product, so that the copy and the three
             kernels run back to back and the interval is their device time, not the enqueue
The colour maps are drawn before the timing (`draw_color_matrix` is a few small numpy products per record; `draw_ms` gives
its host cost per batch for reference). Prints one JSON line. profiles/episode_augment.md was made with it; the plain
figures compare with tools/episode_assembler_bench.py's `assemble` (600 x 600 holders there, 600 x 1000 here)."""
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
         (333, 500, [[20, 30, 300, 300, 2], [100, 150, 320, 330, 1]]),
         ("flip", 0, [[299, 40, 469, 300, 1], [19, 100, 249, 360, 2]]),
         (300, 500, [[60, 50, 400, 290, 1]])]
QUERIES = [dict(row=0, ratio=500 / 375.0, pos_cls=1, order=[2, 0, 1]), dict(row=1, ratio=500 / 333.0, pos_cls=2),
           dict(row=2, ratio=500 / 375.0, pos_cls=2, order=[1, 0]), dict(row=3, ratio=500 / 300.0, pos_cls=1)]
BOXES = [(0, (30, 40, 200, 300)), (1, (100, 150, 320, 330)), (2, (299, 40, 469, 300)), (3, (60, 50, 400, 290)),
         (0, (250, 100, 480, 360)), (1, (20, 30, 300, 300))]
B, WS, TARGET, S, H, W = 4, 6, 600, 320, 600, 1000


class _Count:
    def __init__(self):
        self.n = 0

    def add_call(self, fn, name, args):
        self.n += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    from dana_amd import _lib, pipeline as PL
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(8)
    pool = PL.ImagePool(dev)
    for spec in SPECS:
        if spec[0] == "flip":
            pool.add_flipped(spec[1], spec[2])
        else:
            pool.add(rng.randint(0, 256, size=(spec[0], spec[1], 3)).astype(np.uint8), spec[2])
    pool.freeze()
    sups = [BOXES[(b + k) % 6] for b in range(B) for k in range(WS)]
    draw = np.random.default_rng(5)
    t0 = time.perf_counter()
    for _ in range(50):
        maps = [PL.draw_color_matrix(draw, p=1.0) for _ in range(B + B * WS)]
    draw_ms = (time.perf_counter() - t0) * 1e3 / 50
    aug_queries = [dict(q, color=maps[b], min_visible=0.3) for b, q in enumerate(QUERIES)]
    aug_sups = [s + (maps[B + n],) for n, s in enumerate(sups)]
    holders = {k: PL.EpisodeHolders(B, 2, 3, H, W, dev) for k in ("plain", "augmented")}
    asm = {k: PL.EpisodeAssembler(pool, h, pixel_means=MEANS) for k, h in holders.items()}
    paths = {"plain": lambda: asm["plain"].assemble(PL.plan_episode(pool, QUERIES, sups, holder_hw=(H, W))),
             "augmented": lambda: asm["augmented"].assemble(PL.plan_episode(pool, aug_queries, aug_sups, holder_hw=(H, W)))}
    # identity records through the augmented launches give the plain bits (the tests compare this at edge shapes)
    eye = PL.color_matrix()
    same = asm["augmented"].assemble(PL.plan_episode(pool, [dict(q, color=eye, min_visible=0.0) for q in QUERIES],
                                                     [s + (eye,) for s in sups], holder_hw=(H, W)))
    for a, b in zip(paths["plain"](), same):
        assert torch.equal(a, b), "identity maps through the augmented launches differ from the plain launches"
    launches, words = {}, {}
    for name, fn in paths.items():  # warm-up and the launch counts
        fn()
        _lib.RECORDER = rec = _Count()
        try:
            fn()
        finally:
            _lib.RECORDER = None
        launches[name] = rec.n
    words["plain"] = int(PL.plan_episode(pool, QUERIES, sups, holder_hw=(H, W)).words.nbytes)
    words["augmented"] = int(PL.plan_episode(pool, aug_queries, aug_sups, holder_hw=(H, W)).words.nbytes)
    torch.cuda.synchronize()
    assert not torch.equal(holders["plain"].im_data, holders["augmented"].im_data)
    gpu, host, device = ({k: [] for k in paths} for _ in range(3))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    blocker = torch.randn((8192, 8192), device=dev)
    sink = torch.empty_like(blocker)
    torch.mm(blocker, blocker, out=sink)
    torch.cuda.synchronize()
    done = 0
    while done < args.reps:
        n = min(args.block, args.reps - done)
        for name, fn in paths.items():  # alternating blocks
            for _ in range(n):
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                fn()
                host[name].append((time.perf_counter() - t0) * 1e3)
                e1.record()
                e1.synchronize()
                gpu[name].append(e0.elapsed_time(e1))
            for _ in range(max(n // 4, 1)):
                torch.cuda.synchronize()
                torch.mm(blocker, blocker, out=sink)
                e0.record()  # completes when the product does; the batch is enqueued while it runs
                fn()
                e1.record()
                e1.synchronize()
                device[name].append(e0.elapsed_time(e1))
        done += n
    out = {"label": args.label, "reps": args.reps, "block": args.block,
           "shape": "B %d, way 2, shot 3, holders %dx%d, supports %d" % (B, H, W, S), "pool_bytes": pool.nbytes,
           "draw_ms_per_batch": round(draw_ms, 4)}
    for name in paths:
        g, h, d = np.array(gpu[name]), np.array(host[name]), np.array(device[name])
        out[name] = {"gpu_ms_median": round(float(np.median(g)), 4), "gpu_ms_min": round(float(g.min()), 4),
                     "host_ms_median": round(float(np.median(h)), 4), "host_ms_min": round(float(h.min()), 4),
                     "device_ms_median": round(float(np.median(d)), 4), "device_ms_min": round(float(d.min()), 4),
                     "c_abi_launches": launches[name], "plan_bytes": words[name]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
