"""What the forward-backward check costs a video session per frame: frames.FrameSequence(keypoints=det, tracks=True, fb=...)
against the same session without fb, and the two new launches alone.

    python tools/bench_fb.py [--rounds 5] [--reps 20] [--out profiles/fb_bench.txt]

Everything is measured in ONE process.  FF-RAFT `point` mode, random-init weights, the stream of uint8 (1,H,W,3) frames in
pinned host memory that tools/bench_frame_io.py uses, 384x512 iters 12 and 540x960 iters 32 (padded to 544):
  (a) FrameSequence(keypoints=det, tracks=True).push(frame): one replay, as tools/bench_tracks.py measures it
  (b) the same with fb=FBCheck(): behind the advance the replay also rasterises and pads the backward mask, negates the splatted
      flow, runs the model a second time with as many iterations, and checks every pixel and every slot
  (c) the same with fb=FBCheck(iters=half the iterations)
The three routes alternate inside every round; a round is `reps` pushes and one device synchronisation, ms per frame; medians
over the rounds, all rounds listed.  With random weights another table is another mask and another flow, but the same launches
of the same shapes.  No ratio is fixed in advance; the figures to read are (b) - (a) and (c) - (a) with the spread of the rounds.

Half the iterations change the backward flow, so some verdicts change: for `PAIRS` pairs, each started from an empty table and a
cold forward flow in both sessions (so that the forward flow and the rows are the same), the share of rows with a verdict
(status 1 or 3 under full iterations) whose status differs under half.  With random weights the flow means nothing, so this
says how much the check moves, not how good it is: reported, nothing asserted.

Each new launch alone: 50 calls in one replayed hipGraph between HIP events, so dispatch gaps are included, median of 5
replays, as DESIGN section 4 gives frame_io's figures.  fw is smooth, 3 randn px on a grid of 32 px interpolated bilinearly, as
a real flow is smooth: neighbouring pixels gather from neighbouring taps (white noise as fw would send every lane of a wave to a
line of its own, which no flow does); bw = -fw + 0.5 randn px, so both verdicts occur; 500 rows of which every tenth is no row.  fb_dense's counted bytes are what the
definition has to move at least once, 21 B per pixel: 8 B of fw, 8 B of bw (every element once: what the eight taps ask for beyond
that are lines a neighbour fetches too), 4 B + 1 B out; over the time, as a share of bench.HBM_PEAK_GBS.  At these sizes both
fields fit in the caches, so the share says how far a launch of a few microseconds is from the rate of a long stream."""
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
from focusflow_official_amd.frames import FBCheck, FrameSequence  # noqa: E402
from focusflow_official_amd.keypoints import GoodFeatures  # noqa: E402

CALLS = 50
PAIRS = STREAM - 1
DENSE_BYTES_PER_PIXEL = 8 + 8 + 4 + 1


def launches_alone(dev, h, w, say, replays=5):
    n = 500
    left, top, hp, wp = ops.pad_offsets(h, w)
    g = torch.Generator().manual_seed(0)
    coarse = torch.randn((1, 2, hp // 32 + 2, wp // 32 + 2), generator=g) * 3
    fw = torch.nn.functional.interpolate(coarse, size=(hp, wp), mode="bilinear", align_corners=False).to(dev)
    bw = (-fw.cpu() + torch.randn((1, 2, hp, wp), generator=g) * 0.5).to(dev)
    pts = torch.stack([torch.randint(0, w, (1, n), generator=g), torch.randint(0, h, (1, n), generator=g)], dim=-1).to(torch.int32)
    pts[:, ::10] = -1      # (keypoint_matches passes over a point outside the frame: no row)
    matches, valid0 = ops.keypoint_matches(pts.to(dev), torch.full((1,), n, dtype=torch.int32, device=dev), fw, left, top, h, w)
    valid = valid0.clone()
    out_d = (torch.empty((1, 1, h, w), device=dev), torch.empty((1, 1, h, w), dtype=torch.uint8, device=dev))
    out_m = (torch.empty((1, n), device=dev), torch.empty((1, n), dtype=torch.uint8, device=dev))

    def point_check():
        valid.copy_(valid0)      # (the check clears `valid`: every call starts from the same rows; the copy of 500 bytes is timed too)
        ops.fb_matches(matches, valid, bw, left, top, h, w, out=out_m)

    ops_ = {"fb_dense": lambda: ops.fb_dense(fw, bw, left, top, h, w, out=out_d),
            "fb_matches (N = 500, with a 500-byte copy)": point_check}
    res = {}
    for name, fn in ops_.items():
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(CALLS):
                fn()
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
        res[name] = statistics.median(us)
        say(f"  {name:44s} {res[name]:6.2f} us per call   {[round(x, 2) for x in us]}")
    nbytes = DENSE_BYTES_PER_PIXEL * h * w
    gbs = nbytes / (res["fb_dense"] * 1e-6) / 1e9
    status = torch.bincount(out_m[1].flatten().long(), minlength=4).tolist()
    say(f"  fb_dense: {nbytes / 1e6:.2f} MB counted ({DENSE_BYTES_PER_PIXEL} B per pixel) -> {gbs:.0f} GB/s = {gbs / bench.HBM_PEAK_GBS * 100:.1f} % of "
        f"{bench.HBM_PEAK_GBS:.0f} GB/s; {int(out_d[1].sum())} of {h * w} pixels occluded; status 0 / 1 / 2 / 3 of the rows: {status}")
    res["fb_dense_gbs"], res["fb_dense_frac_of_hbm_peak"] = gbs, gbs / bench.HBM_PEAK_GBS
    return res


def verdicts(full, half, frames):
    """The share of rows with a verdict under full iterations whose status differs under half, over PAIRS independent pairs."""
    rows = differ = 0
    for k in range(PAIRS):
        st = []
        for seq in (full, half):
            seq.reset()
            seq.push(frames[k])
            st.append(seq.push(frames[k + 1]).fb.status.clone())
        judged = (st[0] == 1) | (st[0] == 3)
        rows += int(judged.sum())
        differ += int((judged & (st[0] != st[1])).sum())
    return rows, differ


def section(dev, h, w, iters, rounds, reps, say):
    torch.manual_seed(0)
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=bench.cfg()).to(dev).eval()
    frames = make_stream(h, w)

    def session(fb):
        return FrameSequence(m, raft_iters=iters, keypoints=GoodFeatures(), tracks=True, fb=fb)

    routes = [("(a) FrameSequence(keypoints=det, tracks=True)", session(None)),
              (f"(b) ... fb=FBCheck(): {iters} backward iterations", session(FBCheck())),
              (f"(c) ... fb=FBCheck(iters={iters // 2})", session(FBCheck(iters=iters // 2)))]
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
            if res.fb is not None:
                stats[n[:3]].update(culled=int((res.fb.status == 3).sum()), occluded=int(res.fb.occluded.sum()))
    say(f"FF-RAFT 1x{h}x{w} iters {iters}: ms per frame (median of {rounds} rounds of {reps} frames [all rounds]); last frame: {stats}")
    med = {}
    for n, _ in routes:
        med[n] = statistics.median(times[n])
        say(f"  {n:52s} {med[n]:8.3f} ms   {[round(x, 3) for x in times[n]]}")
    (na, _), (nb, _), (nc, _) = routes
    out = {"tracks_ms": med[na], "fb_ms": med[nb], "fb_half_ms": med[nc], "last_frame": stats}
    spread = max(max(times[n]) - min(times[n]) for n, _ in routes) * 1e3
    for label, n, key in (("(b) - (a)", nb, "fb_diff_us"), ("(c) - (a)", nc, "fb_half_diff_us")):
        diffs = [(y - x) * 1e3 for x, y in zip(times[na], times[n])]
        say(f"  {label} = {(med[n] - med[na]) * 1e3:+.1f} us = {(med[n] - med[na]) / med[na] * 100:+.2f} % of (a); per round {[round(d, 1) for d in diffs]} us")
        out[key], out[key + "_rounds"] = (med[n] - med[na]) * 1e3, diffs
    say(f"  spread between rounds (max - min of one route) {spread:.1f} us")
    out["spread_us"] = spread
    rows, differ = verdicts(routes[1][1], routes[2][1], frames)
    say(f"  verdicts under {iters // 2} backward iterations against {iters}: {differ} of {rows} judged rows differ = {differ / max(rows, 1) * 100:.1f} % "
        f"({PAIRS} pairs from an empty table and a cold start; random weights)")
    out["half_iters_verdicts"] = {"rows": rows, "differ": differ}
    say(f"the new launches alone at 1x{h}x{w} ({CALLS} calls in one replayed graph between events, median of 5 replays):")
    out["alone_us"] = launches_alone(dev, h, w, say)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fb_bench.txt"))
    args = ap.parse_args()
    bench.refuse_lab_switches()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fb.py needs a HIP device (no CPU timing stands in for a GPU measurement)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_fb.py --rounds {args.rounds} --reps {args.reps} on one {torch.cuda.get_device_name(0)} (gfx950)")
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
