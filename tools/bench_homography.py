"""What the homography check costs a video session per frame: frames.FrameSequence(keypoints=det, tracks=True, homography=...)
against the same session without it, and the check's launches alone.

    python tools/bench_homography.py [--rounds 5] [--reps 20] [--out profiles/homography_bench.txt]

Everything is measured in ONE process.  FF-RAFT `point` mode, random-init weights, the stream of uint8 (1,H,W,3) frames in
pinned host memory that tools/bench_frame_io.py uses, 384x512 iters 12 and 540x960 iters 32 (padded to 544):
  (a) FrameSequence(keypoints=det, tracks=True).push(frame): one replay, as tools/bench_tracks.py measures it
  (b) the same with homography=Homography(): behind the advance the replay also copies `valid` (cull is False: the check judges
      a copy) and runs the four launches of csrc/homography.hip, 512 hypotheses over the 500 slots
  (c) the same with homography=Homography(dense=True): also the residual of the cropped flow_up, one more launch over H x W
The routes alternate inside every round; a round is `reps` pushes and one device synchronisation, ms per frame; medians over
the rounds, all rounds listed.  With random weights the flow is no camera's, so the pairs reach no verdict (and the residual is
-1 everywhere: the same bytes written, none of the flow read): the launches and their shapes are what a real stream has, the
dense launch's reads are not, so the residual alone is also timed below with a verdict.  No time is a pass criterion: nothing
comparable exists to hold it against.  The figures to read are (b) - (a) and (c) - (a) next to the spread of the rounds of one
route.

The launches alone: 50 calls in one replayed hipGraph between HIP events, so dispatch gaps are included, median of 5 replays,
as tools/bench_epipolar.py does it: ops.homography_ransac (512 hypotheses) on N = 500 and N = 4096 rows of a synthetic scene
under one homography (a quarter of the matches displaced by 30 px, every tenth row no row), with a 500-byte / 4-KB copy that
puts `valid` back before every call; and ops.homography_residual on an H x W crop of a padded flow with ok = 1, with the bytes
it moves (12 per pixel) and the rate that makes."""
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
from focusflow_official_amd.geometry import Homography  # noqa: E402
from focusflow_official_amd.keypoints import GoodFeatures  # noqa: E402

CALLS = 50
HYPOTHESES = 512


def scene(n, h, w, seed=0):
    """-> ((1,n,4) float32 matches under one homography (a camera that turns and moves in front of a slanted plane), a quarter
    displaced by 30 px, every tenth row no row; the homography (3,3) float32)."""
    rng = np.random.default_rng(seed)
    f = 0.9 * w
    kc = np.array([[f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]])
    rv = rng.uniform(-0.03, 0.03, 3)
    th = np.linalg.norm(rv)
    k = rv / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    rot = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
    hm = kc @ (rot + np.outer(rng.uniform(-0.3, 0.3, 3), [0.2, -0.1, 1.0]) / 5.0) @ np.linalg.inv(kc)
    x = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n), np.ones(n)])
    x2 = hm @ x
    x2 = x2 / x2[2]
    bad = rng.uniform(size=n) < 0.25
    x2[:2, bad] += 30.0 * rng.choice([-1.0, 1.0], (2, n))[:, bad]
    m = np.stack([x[0], x[1], x2[0], x2[1]], 1).astype(np.float32)[None]
    m[:, ::10] = -1
    return m, (hm / hm[2, 2]).astype(np.float32)


def timed_graph(call, replays=5):
    """us per call of CALLS calls in one replayed graph between events: the median, and every replay."""
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
    return statistics.median(us), us


def launches_alone(dev, h, w, say):
    res = {}
    for n in (500, 4096):
        m, _ = scene(n, h, w)
        matches = torch.from_numpy(m).to(dev)
        valid0 = (matches[..., 0] >= 0).to(torch.uint8)
        valid, epoch = valid0.clone(), torch.zeros((), dtype=torch.int32, device=dev)
        ws = torch.empty(ops.homography_ws(1, n, HYPOTHESES), dtype=torch.uint8, device=dev)
        out = ops.homography_ransac(matches, valid, h, w, 1.0, HYPOTHESES, 8, 500, 900, 0, epoch, ws=ws)

        def call():
            valid.copy_(valid0)      # (the check clears `valid`: every call starts from the same rows; the copy is timed too)
            ops.homography_ransac(matches, valid, h, w, 1.0, HYPOTHESES, 8, 500, 900, 0, epoch, out=out, ws=ws)

        med, us = timed_graph(call)
        name = f"homography_ransac (N = {n}, K = {HYPOTHESES}, with a {n}-byte copy)"
        res[name] = med
        status = torch.bincount(out[5].flatten().long(), minlength=5).tolist()
        say(f"  {name:60s} {med:7.2f} us per call   {[round(x, 2) for x in us]}   candidates {int(out[2][0])}, inliers {int(out[1][0])}, "
            f"ok {int(out[3][0])}, planar {int(out[4][0])}, status 0 .. 4 of the rows: {status}")
    # the dense launch with a verdict: the unpadded crop of a padded flow, as the session passes it
    left, top, hp, wp = ops.pad_offsets(h, w, "sintel")
    _, hm = scene(16, h, w)
    flow = torch.randn(1, 2, hp, wp, device=dev)[:, :, top:top + h, left:left + w]
    hm, ok, out = torch.from_numpy(hm).to(dev)[None].contiguous(), torch.ones(1, dtype=torch.uint8, device=dev), torch.empty(1, h, w, device=dev)
    med, us = timed_graph(lambda: ops.homography_residual(flow, hm, ok, out=out))
    name = f"homography_residual ({h}x{w} crop at ({top},{left}) of {hp}x{wp}, ok = 1)"
    res[name] = med
    say(f"  {name:60s} {med:7.2f} us per call   {[round(x, 2) for x in us]}   {12 * h * w / 1e6:.2f} MB moved: {12 * h * w / med / 1e6:.2f} TB/s "
        f"between events, dispatch gaps included; finite values {int(torch.isfinite(out).sum())} of {h * w}")
    return res


def section(dev, h, w, iters, rounds, reps, say):
    torch.manual_seed(0)
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=bench.cfg()).to(dev).eval()
    frames = make_stream(h, w)

    def session(homography):
        return FrameSequence(m, raft_iters=iters, keypoints=GoodFeatures(), tracks=True, homography=homography)

    routes = [("(a) FrameSequence(keypoints=det, tracks=True)", session(None)),
              ("(b) ... homography=Homography()", session(Homography())),
              ("(c) ... homography=Homography(dense=True)", session(Homography(dense=True)))]
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
            if res.hom is not None:
                stats[n[:3]].update(candidates=int(res.hom.candidates[0]), inliers=int(res.hom.inliers[0]), ok=int(res.hom.ok[0]),
                                    planar=int(res.hom.planar[0]))
    say(f"FF-RAFT 1x{h}x{w} iters {iters}: ms per frame (median of {rounds} rounds of {reps} frames [all rounds]); last frame: {stats}")
    med = {}
    for n, _ in routes:
        med[n] = statistics.median(times[n])
        say(f"  {n:56s} {med[n]:8.3f} ms   {[round(x, 3) for x in times[n]]}")
    (na, _), (nb, _), (nc, _) = routes
    out = {"tracks_ms": med[na], "homography_ms": med[nb], "homography_dense_ms": med[nc], "last_frame": stats}
    spread = max(max(times[n]) - min(times[n]) for n, _ in routes) * 1e3
    for label, n, key in (("(b) - (a)", nb, "homography_diff_us"), ("(c) - (a)", nc, "homography_dense_diff_us")):
        diffs = [(y - x) * 1e3 for x, y in zip(times[na], times[n])]
        say(f"  {label} = {(med[n] - med[na]) * 1e3:+.1f} us = {(med[n] - med[na]) / med[na] * 100:+.2f} % of (a); per round {[round(d, 1) for d in diffs]} us")
        out[key], out[key + "_rounds"] = (med[n] - med[na]) * 1e3, diffs
    say(f"  spread between rounds (max - min of one route) {spread:.1f} us")
    out["spread_us"] = spread
    say(f"the check's launches alone at a {h}x{w} frame ({CALLS} calls in one replayed graph between events, median of 5 replays):")
    out["alone_us"] = launches_alone(dev, h, w, say)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_bench.txt"))
    args = ap.parse_args()
    bench.refuse_lab_switches()
    if not torch.cuda.is_available():
        raise SystemExit("bench_homography.py needs a HIP device (no CPU timing stands in for a GPU measurement)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_homography.py --rounds {args.rounds} --reps {args.reps} on one {torch.cuda.get_device_name(0)} (gfx950)")
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
