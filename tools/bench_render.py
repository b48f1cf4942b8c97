"""What flow images cost a video session per frame: frames.FrameSequence(keypoints=det, render=True) against
frames.FrameSequence(keypoints=det), the two new launches alone, and the host route they replace.

    python tools/bench_render.py [--rounds 5] [--reps 20] [--out profiles/render_bench.txt]

Everything is measured in ONE process.  FF-RAFT `point` mode, random-init weights, the stream of uint8 (1,H,W,3) frames in
pinned host memory that tools/bench_frame_io.py uses, 384x512 iters 12 and 540x960 iters 32 (padded to 544):
  (a) FrameSequence(keypoints=det).push(frame): one replay
  (b) FrameSequence(keypoints=det, render=True).push(frame): the same replay with ops.flow_to_image behind the matches: a memset
      node and two launches more (the maximum, the colours), uint8 (1,H,W,3) written into a static buffer
The two routes alternate inside every round; a round is `reps` pushes and one device synchronisation, ms per frame; medians
over the rounds, all rounds listed.  Both sessions run the same launches on the same frames up to the render.  No time is fixed
in advance; the figure to read is (b) - (a) with the spread of the rounds beside it.

The launches alone: 50 calls in one replayed hipGraph between HIP events, so dispatch gaps are included, median of 5 replays,
as DESIGN section 4 gives frame_io's figures: on the padded flow of the stream's last pair, frame at (left, top), into a dense
(1,H,W,3) buffer (the dword stores) and into (1,3,H,W) planes (the byte stores).

The host route this replaces, on the same flow, wall clock with a device synchronisation before and after, median of 5:
  flow_up.cpu()                 the download of the fp32 field, 8 B per pixel, pageable destination as a caller gets it
  + the numpy restatement       tests/flow_viz_ref.py::flow_to_image, which is the reference's flow_viz.flow_to_image byte for byte
and next to it what a consumer of (b) still pays to look at the picture on the host: image.cpu(), 3 B per pixel."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import flow_viz_ref  # noqa: E402
from bench_frame_io import STREAM, make_stream  # noqa: E402
from focusflow_official_amd import FF_RAFT_FUSION, ops  # noqa: E402
from focusflow_official_amd.frames import FrameSequence  # noqa: E402
from focusflow_official_amd.keypoints import GoodFeatures  # noqa: E402

CALLS = 50


def graph_us(fn, replays=5):
    """-> (median, all): us per call of CALLS calls in one replayed graph."""
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
    return statistics.median(us), us


def wall_ms(fn, reps=5):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), ms


def launches_alone(dev, padded, h, w, say):
    left, top, _, _ = ops.pad_offsets(h, w)
    hwc, chw = torch.empty((1, h, w, 3), dtype=torch.uint8, device=dev), torch.empty((1, 3, h, w), dtype=torch.uint8, device=dev)
    rad_max = torch.empty(1, device=dev)
    routes = {"maximum + colours, dense (1,H,W,3) (memset, two launches)": lambda: ops.flow_to_image(padded, left, top, h, w, out=(hwc, rad_max), return_max=True),
              "colours alone, max_flow given, dense (1,H,W,3)": lambda: ops.flow_to_image(padded, left, top, h, w, max_flow=24.0, out=hwc),
              "maximum + colours, planes (1,3,H,W)": lambda: ops.flow_to_image(padded, left, top, h, w, layout="chw", out=(chw, rad_max), return_max=True),
              "colours alone, max_flow given, planes (1,3,H,W)": lambda: ops.flow_to_image(padded, left, top, h, w, max_flow=24.0, layout="chw", out=chw)}
    res = {}
    for name, fn in routes.items():
        res[name], us = graph_us(fn)
        say(f"  {name:62s} {res[name]:7.2f} us per call   {[round(x, 2) for x in us]}")
    return res


def host_route(flow_up, image, say):
    res = {}
    res["flow_up.cpu()"], a = wall_ms(lambda: flow_up.cpu())
    field = flow_up.cpu().numpy()
    res["numpy restatement of flow_to_image"], b = wall_ms(lambda: flow_viz_ref.flow_to_image(field))
    res["image.cpu()"], c = wall_ms(lambda: image.cpu())
    for (name, med), all_ in zip(res.items(), (a, b, c)):
        say(f"  {name:62s} {med:8.3f} ms   {[round(x, 3) for x in all_]}")
    say(f"  host route: flow_up.cpu() + numpy = {res['flow_up.cpu()'] + res['numpy restatement of flow_to_image']:.3f} ms per frame; "
        f"the device route's download: {res['image.cpu()']:.3f} ms")
    return res


def section(dev, h, w, iters, rounds, reps, say):
    torch.manual_seed(0)
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=bench.cfg()).to(dev).eval()
    frames = make_stream(h, w)
    routes = [("(a) FrameSequence(keypoints=det)", FrameSequence(m, raft_iters=iters, keypoints=GoodFeatures())),
              ("(b) FrameSequence(keypoints=det, render=True)", FrameSequence(m, raft_iters=iters, keypoints=GoodFeatures(), render=True))]
    times = {n: [] for n, _ in routes}
    last = {}
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
            last[n] = res
    res_a, res_b = (last[n] for n, _ in routes)
    same = torch.equal(res_a.flow_up, res_b.flow_up)
    say(f"FF-RAFT 1x{h}x{w} iters {iters}: ms per frame (median of {rounds} rounds of {reps} frames [all rounds]); last frame: rad_max "
        f"{float(res_b.view.rad_max[0]):.3f} px, flow_up of (a) and (b) bit-identical: {same}")
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
    padded = res_b.flow_up._base if res_b.flow_up._base is not None else res_b.flow_up      # (flow_up is the crop of the padded field)
    padded = padded.clone()
    say(f"the new launches alone at 1x{h}x{w} ({CALLS} calls in one replayed graph between events, median of 5 replays):")
    alone = launches_alone(dev, padded, h, w, say)
    say(f"the host route at 1x{h}x{w} (wall clock, median of 5):")
    host = host_route(res_b.flow_up, res_b.view.image, say)
    return {"plain_ms": a_ms, "render_ms": b_ms, "diff_us": (b_ms - a_ms) * 1e3, "diff_us_rounds": diffs, "spread_us": spread, "alone_us": alone,
            "host_ms": host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.txt"))
    args = ap.parse_args()
    bench.refuse_lab_switches()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py needs a HIP device (no CPU timing stands in for a GPU measurement)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_render.py --rounds {args.rounds} --reps {args.reps} on one {torch.cuda.get_device_name(0)} (gfx950)")
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
