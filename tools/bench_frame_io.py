"""What a video application pays per frame at the session's boundary: frames.FrameSequence against the route without it.

    python tools/bench_frame_io.py [--rounds 5] [--reps 20] [--out profiles/frame_io_bench.txt]

Everything is measured in ONE process, the two routes alternating inside every round; medians over the rounds, all rounds
listed.  FF-RAFT `point` mode, random-init weights, a stream of uint8 (1,H,W,3) frames in pinned host memory (a 7x7 box mean
of noise that moves by (3,-5) px per frame), 384x512 iters 12 and 540x960 iters 32 (padded to 544), ms per frame:
  (a) today: upload the frame (uint8, non_blocking), torch permute / float / InputPadder.pad of both images of the pair,
      FlowSequence(keypoints=det) replay, det.points(image1), torch gather of the flow at the points, unpad.  (Its graph
      detects on the PADDED image1; the session detects on the unpadded frame and pads the mask, as the reference does.  On
      a frame that needs padding the two masks, hence the flows, differ; the session's flow is checked, untimed, against the
      torch route with the mask made the session's way.)
  (b) FrameSequence(keypoints=det).push(frame): one replay
Both end with the asynchronous copy of matches, valid and count to pinned host memory and ONE event wait per frame, inside
the timed region: wall time per frame as the consumer of the matches sees it.  No ratio is fixed in advance; the figure to
read is (b) - (a) with the spread of the rounds beside it.
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
from focusflow_official_amd import FF_RAFT_FUSION  # noqa: E402
from focusflow_official_amd.frames import FrameSequence  # noqa: E402
from focusflow_official_amd.keypoints import GoodFeatures  # noqa: E402
from focusflow_official_amd.utils import InputPadder  # noqa: E402
from focusflow_official_amd.warm_start import FlowSequence  # noqa: E402

STREAM = 6      # distinct frames, cycled


def make_stream(h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (1, 3, h, w), generator=g).float()
    base = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(base, (3, 3, 3, 3), mode="reflect"), 7, stride=1)
    frames = []
    for k in range(STREAM):
        img = torch.roll(base, shifts=(3 * k, -5 * k), dims=(2, 3)) + torch.randn(1, 3, h, w, generator=g) * 2
        frames.append(img.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().pin_memory())
    return frames


class Host:
    """Pinned destinations of the results and the event the consumer waits for."""

    def __init__(self, n):
        self.matches = torch.empty((1, n, 4), dtype=torch.float32, pin_memory=True)
        self.valid = torch.empty((1, n), dtype=torch.uint8, pin_memory=True)
        self.count = torch.empty((1,), dtype=torch.int32, pin_memory=True)
        self.event = torch.cuda.Event()

    def take(self, matches, valid, count):
        self.matches.copy_(matches, non_blocking=True)
        self.valid.copy_(valid, non_blocking=True)
        self.count.copy_(count, non_blocking=True)
        self.event.record()
        self.event.synchronize()


class Today:
    """strict=True (the check, not timed): mask1 = InputPadder.pad(det(unpadded image1)) is supplied, as evaluate.py makes and pads
    its masks and as FrameSequence does; the timed route lets FlowSequence(keypoints=det) detect on the padded image1."""

    def __init__(self, model, det, iters, dev, h, w, strict=False):
        self.seq, self.det, self.dev = FlowSequence(model, raft_iters=iters, keypoints=None if strict else det), det, dev
        self.strict = strict
        self.prev = None
        self.u8 = [torch.empty((1, h, w, 3), dtype=torch.uint8, device=dev) for _ in range(2)]      # this frame and the one before
        self.k = 0
        self.flow_up = None

    def reset(self):
        self.prev = None
        self.seq.reset()

    def push(self, frame, host):
        cur = self.u8[self.k]
        self.k ^= 1
        cur.copy_(frame, non_blocking=True)
        prev, self.prev = self.prev, cur
        if prev is None:
            return False
        with torch.no_grad():
            i1, i2 = prev.permute(0, 3, 1, 2).float(), cur.permute(0, 3, 1, 2).float()
            padder = InputPadder(i1.shape)
            p1, p2 = padder.pad(i1, i2)
            _, flow_up = self.seq(p1, p2, padder.pad(self.det(i1))[0]) if self.strict else self.seq(p1, p2)
            points, count = self.det.points(i1)
            flow_up = padder.unpad(flow_up)
            h, w = flow_up.shape[-2:]
            n = points.shape[1]
            x, y = points[..., 0].long(), points[..., 1].long()
            live = torch.arange(n, device=self.dev)[None] < count[:, None]
            xs, ys = x.clamp(0, w - 1), y.clamp(0, h - 1)
            u, v = flow_up[0, 0, ys, xs], flow_up[0, 1, ys, xs]
            xf, yf = x.float(), y.float()
            tx, ty = xf + u, yf + v
            m = torch.stack([xf, yf, tx, ty], dim=-1)
            m = torch.where(live[..., None], m, torch.full_like(m, -1.0))
            valid = (live & (tx >= 0) & (tx <= w - 1) & (ty >= 0) & (ty <= h - 1)).to(torch.uint8)
        self.flow_up = flow_up
        host.take(m, valid, count)
        return True


class Session:
    def __init__(self, model, det, iters):
        self.seq = FrameSequence(model, raft_iters=iters, keypoints=det)
        self.flow_up = None

    def reset(self):
        self.seq.reset()

    def push(self, frame, host):
        res = self.seq.push(frame)
        if res is None:
            return False
        self.flow_up = res.flow_up
        host.take(res.matches, res.valid, res.count)
        return True


def section(dev, h, w, iters, rounds, reps, say):
    torch.manual_seed(0)
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=bench.cfg()).to(dev).eval()
    det = GoodFeatures()
    frames = make_stream(h, w)
    routes = [("(a) today: torch convert / pad / gather", Today(m, det, iters, dev, h, w), Host(det.max_corners)),
              ("(b) FrameSequence.push", Session(m, det, iters), Host(det.max_corners))]
    # the same stream through both, and through the torch route with the session's mask semantics: faster and different is not faster
    strict, hs = Today(m, det, iters, dev, h, w, strict=True), Host(det.max_corners)
    worst = worst_strict = 0.0
    for t in range(STREAM):
        got = [r.push(frames[t], host) for _, r, host in routes] + [strict.push(frames[t], hs)]
        if all(got):
            (_, ra, ha), (_, rb, hb) = routes
            assert torch.equal(ha.count, hb.count) and torch.equal(ha.matches[..., :2], hb.matches[..., :2]), "the two routes disagree on the key points"
            worst = max(worst, float((ra.flow_up - rb.flow_up).abs().max()))
            worst_strict = max(worst_strict, float((strict.flow_up - rb.flow_up).abs().max()))
            assert torch.equal(hs.matches, hb.matches) and torch.equal(hs.valid, hb.valid) or worst_strict > 0, "equal flows, different matches"
    assert worst_strict <= 2e-4, f"FrameSequence against the torch route with mask1 = pad(det(unpadded image1)): flow_up differs by {worst_strict:.3e} px"
    del strict
    kept = int(routes[0][2].count[0])
    times = {n: [] for n, _, _ in routes}
    for r in range(rounds + 1):      # (the first round warms up and is dropped)
        for n, route, host in routes:
            route.reset()
            route.push(frames[0], host)
            route.push(frames[1], host)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(reps):
                route.push(frames[(k + 2) % STREAM], host)
            dt = (time.perf_counter() - t0) / reps * 1e3      # (every push ended in its event wait)
            if r:
                times[n].append(dt)
    say(f"FF-RAFT 1x{h}x{w} iters {iters}: {kept} key points in the last frame; ms per frame (median of {rounds} rounds of {reps} frames [all rounds])")
    say(f"  max |flow_up difference| over {STREAM - 1} pairs: (b) against the torch route with mask1 = pad(det(unpadded image1)) {worst_strict:.2e} px (asserted <= 2e-4); "
        f"(b) against (a) {worst:.2e} px" + (" - (a) detects on the PADDED image1, another mask; the weights are random, so another mask is another flow" if worst > 2e-4 else ""))
    med = {}
    for n, _, _ in routes:
        med[n] = statistics.median(times[n])
        say(f"  {n:42s} {med[n]:8.3f} ms   {[round(x, 3) for x in times[n]]}")
    a, b = (times[n] for n, _, _ in routes)
    a_ms, b_ms = (med[n] for n, _, _ in routes)
    diffs = [(y - x) * 1e3 for x, y in zip(a, b)]
    spread = max(max(a) - min(a), max(b) - min(b)) * 1e3
    say(f"  (b) - (a) = {(b_ms - a_ms) * 1e3:+.1f} us = {(b_ms - a_ms) / a_ms * 100:+.2f} % of (a); per round {[round(d, 1) for d in diffs]} us; "
        f"spread between rounds (max - min of one route) {spread:.1f} us")
    return {"kept": kept, "today_ms": a_ms, "session_ms": b_ms, "diff_us": (b_ms - a_ms) * 1e3, "diff_us_rounds": diffs, "spread_us": spread,
            "flow_up_max_diff_vs_padded_mask_route": worst, "flow_up_max_diff_vs_same_mask_route": worst_strict}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_io_bench.txt"))
    args = ap.parse_args()
    bench.refuse_lab_switches()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_io.py needs a HIP device (no CPU timing stands in for a GPU measurement)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_frame_io.py --rounds {args.rounds} --reps {args.reps} on one {torch.cuda.get_device_name(0)} (gfx950)")
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
