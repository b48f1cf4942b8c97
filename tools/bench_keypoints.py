"""What detecting key points inside the video graph costs (csrc/keypoints.hip, FlowSequence(keypoints=...)).

    python tools/bench_keypoints.py [--rounds 5] [--reps 20] [--out profiles/keypoints_bench.txt]

Everything is measured in ONE process, the variants alternating inside every round; medians over the rounds, all rounds
listed.  FF-RAFT `point` mode, random-init weights, 1x384x512 iters 12 and 1x544x960 iters 32, ms per pair:
  (a) FlowSequence replay with a caller-supplied device mask that already lies in the graph's mask1 buffer (no copy):
      the mask costs nothing - the floor
  (b) FlowSequence(keypoints=GoodFeatures()) replay: the detector runs inside the graph
  (c) the detector's launches alone: 20 calls captured into one hipGraph, the replay bracketed by HIP events
on uniform noise (every fourth pixel a 3x3 maximum: the worst case for the distance rounds) and on the same noise under a
7x7 box mean.  The figure to read is (b) - (a), with the spread of the rounds beside it.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from focusflow_official_amd import FF_RAFT_FUSION, ops  # noqa: E402
from focusflow_official_amd.keypoints import GoodFeatures  # noqa: E402
from focusflow_official_amd.warm_start import FlowSequence  # noqa: E402

CALLS = 20


def make_pair(kind, h, w, dev, seed=0):
    """R,G,B frames of integers 0..255: uniform noise, or its 7x7 box mean (reflect padding, rounded); frame 2 = frame 1
    moved by (3, -5) px plus noise, as bench.synthetic_batch makes it."""
    g = torch.Generator().manual_seed(seed)
    i1 = torch.randint(0, 256, (1, 3, h, w), generator=g).float()
    if kind == "blur7x7":
        i1 = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(i1, (3, 3, 3, 3), mode="reflect"), 7, stride=1).round()
    i2 = (torch.roll(i1, shifts=(3, -5), dims=(2, 3)) + torch.randn(1, 3, h, w, generator=g) * 2).clamp(0, 255)
    return i1.contiguous().to(dev), i2.contiguous().to(dev)


def section(dev, h, w, iters, rounds, reps, say):
    torch.manual_seed(0)
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=bench.cfg()).to(dev).eval()
    det = GoodFeatures()
    res = {}
    for kind in ("noise", "blur7x7"):
        i1, i2 = make_pair(kind, h, w, dev)
        mask, _, count = ops.good_features(i1, return_points=True)
        n_kept = int(count[0])
        supplied = FlowSequence(m, raft_iters=iters)
        detecting = FlowSequence(m, raft_iters=iters, keypoints=det)
        out = torch.empty_like(mask)
        torch.cuda.synchronize()
        alone = torch.cuda.CUDAGraph()
        with torch.cuda.graph(alone):
            for _ in range(CALLS):
                det(i1, out=out)

        supplied(i1, i2, mask)                      # (captures)
        static_mask = supplied._graphed.mask1       # the graph's own mask1 buffer: passing it back costs no copy
        static_mask.copy_(mask)

        def run_supplied():
            supplied(i1, i2, static_mask)

        def run_detecting():
            detecting(i1, i2)

        variants = [("(a) replay, mask supplied", run_supplied), ("(b) replay, detector in the graph", run_detecting)]
        times = {n: [] for n, _ in variants}
        alone_us = []
        for r in range(rounds + 1):      # (the first round warms up and is dropped)
            for n, fn in variants:
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                if r:
                    times[n].append((time.perf_counter() - t0) / reps * 1e3)
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            alone.replay()
            z.record()
            z.synchronize()
            if r:
                alone_us.append(a.elapsed_time(z) * 1e3 / CALLS)
        assert torch.equal(detecting.mask1, mask) and torch.equal(out, mask)      # faster and different is not faster
        say(f"FF-RAFT 1x{h}x{w} iters {iters}, {kind}: {n_kept} key points kept; ms per pair (median of {rounds} rounds of {reps} pairs [all rounds])")
        med = {}
        for n, _ in variants:
            med[n] = statistics.median(times[n])
            say(f"  {n:36s} {med[n]:8.3f} ms   {[round(x, 3) for x in times[n]]}")
        a_ms, b_ms = med[variants[0][0]], med[variants[1][0]]
        diffs = [(y - x) * 1e3 for x, y in zip(times[variants[0][0]], times[variants[1][0]])]
        say(f"  (b) - (a) = {(b_ms - a_ms) * 1e3:+.1f} us = {(b_ms - a_ms) / a_ms * 100:+.2f} % of (a); per round {[round(d, 1) for d in diffs]} us")
        say(f"  (c) detector alone                  {statistics.median(alone_us):8.1f} us per call ({CALLS} calls per replayed graph, HIP events)   {[round(x, 1) for x in alone_us]}")
        res[kind] = {"kept": n_kept, "supplied_ms": a_ms, "detecting_ms": b_ms, "added_us": (b_ms - a_ms) * 1e3, "added_us_rounds": diffs,
                     "alone_us": statistics.median(alone_us)}
        del supplied, detecting, alone
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoints_bench.txt"))
    args = ap.parse_args()
    bench.refuse_lab_switches()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keypoints.py needs a HIP device (no CPU timing stands in for a GPU measurement)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_keypoints.py --rounds {args.rounds} --reps {args.reps} on one {torch.cuda.get_device_name(0)} (gfx950)")
    out = {"device": torch.cuda.get_device_name(0)}
    out["pair_384x512_it12"] = section(dev, 384, 512, 12, args.rounds, args.reps, say)
    out["pair_544x960_it32"] = section(dev, 544, 960, 32, args.rounds, max(args.reps // 2, 1), say)
    torch.cuda.synchronize()
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
