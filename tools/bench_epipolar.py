"""What the epipolar check costs a video session per frame: frames.FrameSequence(keypoints=det, tracks=True, epipolar=...) against
the same session without it, and the check's launches alone.

    python tools/bench_epipolar.py [--rounds 5] [--reps 20] [--out profiles/epipolar_bench.txt]

Everything is measured in ONE process.  FF-RAFT `point` mode, random-init weights, the stream of uint8 (1,H,W,3) frames in
pinned host memory that tools/bench_frame_io.py uses, 384x512 iters 12 and 540x960 iters 32 (padded to 544):
  (a) FrameSequence(keypoints=det, tracks=True).push(frame): one replay, as tools/bench_tracks.py measures it
  (b) the same with epipolar=Epipolar(): behind the advance the replay also runs the four launches of csrc/epipolar.hip, 512
      hypotheses over the 500 slots
  (c) the same with epipolar=Epipolar(min_inliers=8, min_ratio=0): the same launches, but every pair gets a verdict and its
      outliers are culled, so the next replenish has slots to refill
The routes alternate inside every round; a round is `reps` pushes and one device synchronisation, ms per frame; medians over
the rounds, all rounds listed.  With random weights the flow is no camera's, so (b) reaches no verdict and (c) culls nearly
everything: another table is another mask and another flow, but the same launches of the same shapes.  No time is a pass
criterion: nothing comparable exists to hold it against.  The figures to read are (b) - (a) and (c) - (a) next to the spread of
the rounds of one route.

The launches alone: 50 calls of ops.epipolar_ransac (512 hypotheses) in one replayed hipGraph between HIP events, so dispatch
gaps are included, median of 5 replays, as DESIGN section 4 gives frame_io's figures; N = 500 and N = 4096 rows of a synthetic
two-view scene (a pinhole camera that turns and moves over points of depth 2 .. 12; a quarter of the matches displaced by 30 px,
every tenth row no row), with a 500-byte / 4-KB copy that puts `valid` back before every call."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from bench_frame_io import STREAM, make_stream  # noqa: E402
from focusflow_official_amd import FF_RAFT_FUSION, ops  # noqa: E402
from focusflow_official_amd.frames import FrameSequence  # noqa: E402
from focusflow_official_amd.geometry import Epipolar  # noqa: E402
from focusflow_official_amd.keypoints import GoodFeatures  # noqa: E402

CALLS = 50
HYPOTHESES = 512


def scene(n, h, w, seed=0):
    """(1,n,4) float32 matches of a camera that turns by a few hundredths of a radian and moves; a quarter displaced by 30 px."""
    rng = np.random.default_rng(seed)
    f = 0.9 * w
    kc = np.array([[f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]])
    x = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n), np.ones(n)])
    pts = np.linalg.inv(kc) @ x * rng.uniform(2, 12, n)
    rv = rng.uniform(-0.03, 0.03, 3)
    th = np.linalg.norm(rv)
    k = rv / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    rot = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
    x2 = kc @ (rot @ pts + rng.uniform(-0.3, 0.3, 3)[:, None])
    x2 = x2 / x2[2]
    bad = rng.uniform(size=n) < 0.25
    x2[:2, bad] += 30.0 * rng.choice([-1.0, 1.0], (2, n))[:, bad]
    m = np.stack([x[0], x[1], x2[0], x2[1]], 1).astype(np.float32)[None]
    m[:, ::10] = -1
    return m


def launches_alone(dev, h, w, say, replays=5):
    res = {}
    for n in (500, 4096):
        matches = torch.from_numpy(scene(n, h, w)).to(dev)
        valid0 = (matches[..., 0] >= 0).to(torch.uint8)
        valid, epoch = valid0.clone(), torch.zeros((), dtype=torch.int32, device=dev)
        ws = torch.empty(ops.epipolar_ws(1, n, HYPOTHESES), dtype=torch.uint8, device=dev)
        out = ops.epipolar_ransac(matches, valid, h, w, 1.0, HYPOTHESES, 16, 500, 0, epoch, ws=ws)

        def call():
            valid.copy_(valid0)      # (the check clears `valid`: every call starts from the same rows; the copy is timed too)
            ops.epipolar_ransac(matches, valid, h, w, 1.0, HYPOTHESES, 16, 500, 0, epoch, out=out, ws=ws)

        call()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(CALLS):
                call()
        graph.replay()
        torch.cuda.synchronize()
        us = []
        for _ in range(replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / CALLS)
        name = f"epipolar_ransac (N = {n}, K = {HYPOTHESES}, with a {n}-byte copy)"
        res[name] = statistics.median(us)
        status = torch.bincount(out[4].flatten().long(), minlength=5).tolist()
        say(f"  {name:58s} {res[name]:7.2f} us per call   {[round(x, 2) for x in us]}   candidates {int(out[2][0])}, inliers {int(out[1][0])}, "
            f"ok {int(out[3][0])}, status 0 .. 4 of the rows: {status}")
    return res


def section(dev, h, w, iters, rounds, reps, say):
    torch.manual_seed(0)
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=bench.cfg()).to(dev).eval()
    frames = make_stream(h, w)

    def session(epipolar):
        return FrameSequence(m, raft_iters=iters, keypoints=GoodFeatures(), tracks=True, epipolar=epipolar)

    routes = [("(a) FrameSequence(keypoints=det, tracks=True)", session(None)),
              ("(b) ... epipolar=Epipolar()", session(Epipolar())),
              ("(c) ... epipolar=Epipolar(min_inliers=8, min_ratio=0)", session(Epipolar(min_inliers=8, min_ratio=0.0)))]
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
            stats[n[:3]] = {"live": int(res.count[0]), "born": int(res.tracks.born[0]), "max_age": int(res.tracks.age.max()), "valid": int(res.valid.sum())}
            if res.epi is not None:
                stats[n[:3]].update(candidates=int(res.epi.candidates[0]), inliers=int(res.epi.inliers[0]), ok=int(res.epi.ok[0]),
                                    culled=int((res.epi.status == 3).sum()))
    say(f"FF-RAFT 1x{h}x{w} iters {iters}: ms per frame (median of {rounds} rounds of {reps} frames [all rounds]); last frame: {stats}")
    med = {}
    for n, _ in routes:
        med[n] = statistics.median(times[n])
        say(f"  {n:56s} {med[n]:8.3f} ms   {[round(x, 3) for x in times[n]]}")
    (na, _), (nb, _), (nc, _) = routes
    out = {"tracks_ms": med[na], "epipolar_ms": med[nb], "epipolar_culling_ms": med[nc], "last_frame": stats}
    spread = max(max(times[n]) - min(times[n]) for n, _ in routes) * 1e3
    for label, n, key in (("(b) - (a)", nb, "epipolar_diff_us"), ("(c) - (a)", nc, "epipolar_culling_diff_us")):
        diffs = [(y - x) * 1e3 for x, y in zip(times[na], times[n])]
        say(f"  {label} = {(med[n] - med[na]) * 1e3:+.1f} us = {(med[n] - med[na]) / med[na] * 100:+.2f} % of (a); per round {[round(d, 1) for d in diffs]} us")
        out[key], out[key + "_rounds"] = (med[n] - med[na]) * 1e3, diffs
    say(f"  spread between rounds (max - min of one route) {spread:.1f} us")
    out["spread_us"] = spread
    say(f"the check's four launches alone at a {h}x{w} frame ({CALLS} calls in one replayed graph between events, median of 5 replays):")
    out["alone_us"] = launches_alone(dev, h, w, say)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epipolar_bench.txt"))
    args = ap.parse_args()
    bench.refuse_lab_switches()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epipolar.py needs a HIP device (no CPU timing stands in for a GPU measurement)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_epipolar.py --rounds {args.rounds} --reps {args.reps} on one {torch.cuda.get_device_name(0)} (gfx950)")
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
