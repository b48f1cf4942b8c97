"""What key-point tracks cost a video session per frame: frames.FrameSequence(keypoints=det, tracks=True) against
frames.FrameSequence(keypoints=det), and the three new launches alone.

    python tools/bench_tracks.py [--rounds 5] [--reps 20] [--out profiles/tracks_bench.txt]

Everything is measured in ONE process.  FF-RAFT `point` mode, random-init weights, the stream of uint8 (1,H,W,3) frames in
pinned host memory that tools/bench_frame_io.py uses, 384x512 iters 12 and 540x960 iters 32 (padded to 544):
  (a) FrameSequence(keypoints=det).push(frame): one replay (detect, pad the mask, forward, forward_interpolate, matches)
  (b) FrameSequence(keypoints=det, tracks=True).push(frame): one replay (detect, replenish, mask, pad, forward,
      forward_interpolate, advance): three launches more (replenish, zero, scatter), advance in the place of matches
The two routes alternate inside every round; a round is `reps` pushes and one device synchronisation, ms per frame; medians
over the rounds, all rounds listed.  In (b) the model reads the rasterised tracks as mask1, in (a) the detector's mask:
with random weights another mask is another flow, but the same launches of the same shapes.  No ratio is fixed in advance;
the figure to read is (b) - (a) with the spread of the rounds beside it.

Each new launch alone: 50 calls in one replayed hipGraph between HIP events, so dispatch gaps are included, median of 5
replays, as DESIGN section 4 gives frame_io's figures.  The table is in a steady state there: N = M = 500; 400 tracks lie a
quarter pixel off the first 400 detections, and the first (untimed) replay gives birth to those of the other 100 detections
that no track blocks, so from then on every detection is blocked and all 50 calls do the same work.  How many tracks are
live then depends on the frame size (the larger the frame, the fewer of the 100 are blocked): the output states the count.
The advance runs on a zero flow (the tracks stay where they are and age)."""
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
from bench_frame_io import STREAM, make_stream  # noqa: E402
from focusflow_official_amd import FF_RAFT_FUSION, ops  # noqa: E402
from focusflow_official_amd.frames import FrameSequence  # noqa: E402
from focusflow_official_amd.keypoints import GoodFeatures  # noqa: E402
from focusflow_official_amd.tracks import TrackTable  # noqa: E402

CALLS = 50


def launches_alone(dev, h, w, say, replays=5):
    n = m = 500
    left, top, hp, wp = ops.pad_offsets(h, w)
    g = torch.Generator().manual_seed(0)
    pts = torch.stack([torch.randint(0, w, (1, m), generator=g), torch.randint(0, h, (1, m), generator=g)], dim=-1).to(torch.int32).to(dev)
    count = torch.full((1,), m, dtype=torch.int32, device=dev)
    tb = TrackTable(1, n, dev)
    tb.pos[:, :400] = pts[:, :400].float() + 0.25      # 400 live tracks a quarter pixel off their detections
    tb.ids[:, :400] = torch.arange(400, device=dev)
    flow = torch.zeros((1, 2, hp, wp), device=dev)
    mask = torch.empty((1, 1, h, w), device=dev)
    out_r = (torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    out_a = (torch.empty((1, n, 4), device=dev), torch.empty((1, n), dtype=torch.uint8, device=dev),
             torch.empty((1, n), dtype=torch.int64, device=dev), torch.empty((1, n), dtype=torch.int32, device=dev))
    ops_ = {"replenish (N = M = 500)": lambda: ops.tracks_replenish(tb.pos, tb.ids, tb.age, tb.next_id, pts, count, h, w, 10, out=out_r),
            "mask (zero + scatter: two launches)": lambda: ops.tracks_mask(tb.pos, tb.ids, h, w, out=mask),
            "advance (N = 500)": lambda: ops.tracks_advance(tb.pos, tb.ids, tb.age, flow, left, top, h, w, out=out_a)}
    res = {}
    for name, fn in ops_.items():
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(CALLS):
                fn()
        graph.replay()      # (untimed: the first replenish fills the free slots)
        torch.cuda.synchronize()
        us = []
        for _ in range(replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / CALLS)
        res[name] = statistics.median(us)
        say(f"  {name:38s} {res[name]:6.2f} us per call   {[round(x, 2) for x in us]}")
    say(f"  (steady state: {int(tb.live.sum())} of {n} slots live, next_id {int(tb.next_id[0])})")
    return res


def section(dev, h, w, iters, rounds, reps, say):
    torch.manual_seed(0)
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=bench.cfg()).to(dev).eval()
    frames = make_stream(h, w)
    routes = [("(a) FrameSequence(keypoints=det)", FrameSequence(m, raft_iters=iters, keypoints=GoodFeatures())),
              ("(b) FrameSequence(keypoints=det, tracks=True)", FrameSequence(m, raft_iters=iters, keypoints=GoodFeatures(), tracks=True))]
    times = {n: [] for n, _ in routes}
    stats = {}
    for r in range(rounds + 1):      # (the first round captures, warms up and is dropped)
        for n, seq in routes:
            seq.reset()
            seq.push(frames[0])
            seq.push(frames[1])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(reps):
                res = seq.push(frames[(k + 2) % STREAM])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / reps * 1e3
            if r:
                times[n].append(dt)
            if res.tracks is not None:
                stats = {"live": int(res.count[0]), "born": int(res.tracks.born[0]), "max_age": int(res.tracks.age.max()), "valid": int(res.valid.sum())}
            else:
                stats["detected"] = int(res.count[0])
    say(f"FF-RAFT 1x{h}x{w} iters {iters}: ms per frame (median of {rounds} rounds of {reps} frames [all rounds]); last frame: {stats}")
    med = {}
    for n, _ in routes:
        med[n] = statistics.median(times[n])
        say(f"  {n:46s} {med[n]:8.3f} ms   {[round(x, 3) for x in times[n]]}")
    a, b = (times[n] for n, _ in routes)
    a_ms, b_ms = (med[n] for n, _ in routes)
    diffs = [(y - x) * 1e3 for x, y in zip(a, b)]
    spread = max(max(a) - min(a), max(b) - min(b)) * 1e3
    say(f"  (b) - (a) = {(b_ms - a_ms) * 1e3:+.1f} us = {(b_ms - a_ms) / a_ms * 100:+.2f} % of (a); per round {[round(d, 1) for d in diffs]} us; "
        f"spread between rounds (max - min of one route) {spread:.1f} us")
    say(f"the new launches alone at 1x{h}x{w} ({CALLS} calls in one replayed graph between events, median of 5 replays):")
    alone = launches_alone(dev, h, w, say)
    return {"plain_ms": a_ms, "tracks_ms": b_ms, "diff_us": (b_ms - a_ms) * 1e3, "diff_us_rounds": diffs, "spread_us": spread, "last_frame": stats,
            "alone_us": alone}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_bench.txt"))
    args = ap.parse_args()
    bench.refuse_lab_switches()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tracks.py needs a HIP device (no CPU timing stands in for a GPU measurement)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_tracks.py --rounds {args.rounds} --reps {args.reps} on one {torch.cuda.get_device_name(0)} (gfx950)")
    out = {"device": torch.cuda.get_device_name(0)}
    out["stream_384x512_it12"] = section(dev, 384, 512, 12, args.rounds, args.reps, say)
    out["stream_540x960_it32"] = section(dev, 540, 960, 32, args.rounds, max(args.reps // 2, 1), say)
    torch.cuda.synchronize()
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
