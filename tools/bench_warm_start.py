"""What warm-start video inference costs (csrc/warm_start.hip, graph.GraphedForward(warm_start=True), warm_start.FlowSequence).

    python tools/bench_warm_start.py [--rounds 5] [--out profiles/warm_start_bench.txt] [--bench-parent DIR]

Everything is measured in ONE process, the variants alternating inside every round; medians over the rounds, all rounds
listed.
  kernel   ff_forward_interpolate alone (five launches): 20 calls captured into one hipGraph, the replay bracketed by HIP
           events (no host issue time in the figure), B = 1 / 8, four planes, randn*2 and a smooth +-6 px field; the landed
           fraction beside each figure, since a binned search depends on the distribution
  per pair FF-RAFT 1x384x512 iters 12 and 1x544x960 iters 32 (random-init weights, bench.py's synthetic pair), ms per pair:
           (i)   the captured cold forward (GraphedForward)
           (ii)  warm start without this kernel: eager forward with flow_init + utils.forward_interpolate on the host (scipy)
                 + the two copies
           (iii) FlowSequence(graph=True)
  bench    --bench-parent DIR: bench.py's default line from this tree and from a built checkout of the parent commit in DIR,
           alternating, each in a child process of its own
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from focusflow_official_amd import FF_RAFT_FUSION, ops, utils  # noqa: E402
from focusflow_official_amd.graph import GraphedForward  # noqa: E402
from focusflow_official_amd.warm_start import FlowSequence  # noqa: E402

# utils.forward_interpolate's scipy part alone, measured on the CPU of the authoring container (used only where scipy is missing)
HOST_STAND_IN = "5-6 ms for a 46x62 / 48x64 plane, 12-17 ms for 68x120"
PLANES = [(48, 64), (68, 120), (136, 240), (270, 480)]
CALLS = 20


def landed_fraction(f):
    _, _, h, w = f.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=f.device), torch.arange(w, device=f.device), indexing="ij")
    x1, y1 = xs.double() + f[:, 0].double(), ys.double() + f[:, 1].double()
    return float(((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)).double().mean())


def make_flow(kind, b, h, w, dev, g):
    if kind == "randn*2":
        return (torch.randn(b, 2, h, w, generator=g) * 2).to(dev)
    f = torch.nn.functional.interpolate(torch.randn(b, 2, h // 8 + 2, w // 8 + 2, generator=g), size=(h, w), mode="bicubic", align_corners=False)
    return (f * (6.0 / f.abs().max())).to(dev)


def kernel_section(dev, rounds, say):
    g = torch.Generator().manual_seed(0)
    cases = []
    for b in (1, 8):
        for h, w in PLANES:
            for kind in ("randn*2", "smooth"):
                f = make_flow(kind, b, h, w, dev, g)
                out = torch.empty_like(f)
                ops.forward_interpolate(f, out=out)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for _ in range(CALLS):
                        ops.forward_interpolate(f, out=out)
                cases.append((f"B={b} {h}x{w} {kind}", landed_fraction(f), graph, [], (f, out)))
    for _ in range(rounds + 1):      # (the first round warms up and is dropped)
        for _, _, graph, times, _ in cases:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            z.record()
            z.synchronize()
            times.append(a.elapsed_time(z) * 1e3 / CALLS)
    say(f"ff_forward_interpolate alone, us per call ({CALLS} calls per replayed graph, HIP events; median of {rounds} rounds [all rounds])")
    res = {}
    for name, frac, _, times, _ in cases:
        t = times[1:]
        res[name] = {"us": statistics.median(t), "landed": frac}
        say(f"  {name:26s} landed {frac:5.3f}   {statistics.median(t):8.1f} us   {[round(x, 1) for x in t]}")
    return res


def pair_section(dev, h, w, iters, rounds, reps, have_scipy, say):
    torch.manual_seed(0)
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=bench.cfg()).to(dev).eval()
    batch = bench.synthetic_batch(1, h, w, 1, dev)
    cold = GraphedForward(m, batch, raft_iters=iters)
    seq = FlowSequence(m, raft_iters=iters, graph=True)
    state = {"finit": None}

    def run_cold():
        cold(*batch)

    def run_seq():
        seq(*batch)

    def run_host():
        with torch.no_grad():
            low, _ = m(*batch, raft_iters=iters, flow_init=state["finit"], test_mode=True)
        state["finit"] = utils.forward_interpolate(low[0])[None].to(dev)      # (device -> host with a sync, scipy, host -> device)

    variants = [("(i) captured cold forward", run_cold), ("(iii) FlowSequence(graph=True)", run_seq)]
    if have_scipy:
        variants.append(("(ii) eager + flow_init + host forward_interpolate", run_host))
    times = {n: [] for n, _ in variants}
    for r in range(rounds + 1):
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
    low = seq(*batch)[0]
    say(f"FF-RAFT 1x{h}x{w} iters {iters}, ms per pair (median of {rounds} rounds of {reps} pairs [all rounds]); "
        f"flow_low of the warm-started pair: landed {landed_fraction(low):.3f}, max |flow| {float(low.abs().max()):.2f}")
    med = {}
    for n, _ in variants:
        med[n] = statistics.median(times[n])
        say(f"  {n:52s} {med[n]:8.3f} ms   {[round(x, 3) for x in times[n]]}")
    i, iii = med[variants[0][0]], med[variants[1][0]]
    say(f"  (iii) - (i)  = {(iii - i) * 1e3:+.1f} us = {(iii - i) / i * 100:+.2f} % of (i)     what warm start adds to a replay")
    if have_scipy:
        ii = med[variants[2][0]]
        say(f"  (ii) - (iii) = {ii - iii:+.3f} ms                          what the host route cost")
    else:
        say(f"  (ii) not measured: scipy is not importable here.  Stand-in (CPU of the authoring container, the scipy part alone): {HOST_STAND_IN}")
    return med


def bench_section(parent, rounds, say):
    say("bench.py --gpus 1 --steps 10 --warmup 3, this tree and a checkout of the parent commit alternating, one child process each")
    res = {"this": [], "parent": []}
    for _ in range(rounds):
        for name, cwd in (("this", ROOT), ("parent", parent)):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3"], cwd=cwd, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:      # (nothing more is started on the GPU after a failure)
                raise SystemExit(f"bench.py failed in {cwd} ({p.returncode}):\n{p.stderr[-2000:]}")
            line = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
            res[name].append(line["value"])
            say(f"  {name:6s} {line['value']:9.3f} {line['unit']}   ({line['ms_per_step']} ms per step)")
    say(f"  medians: this {statistics.median(res['this']):.3f}, parent {statistics.median(res['parent']):.3f}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warm_start_bench.txt"))
    ap.add_argument("--bench-parent", metavar="DIR", help="a built checkout of the parent commit: also compare bench.py's default line")
    args = ap.parse_args()
    bench.refuse_lab_switches()
    if not torch.cuda.is_available():
        raise SystemExit("bench_warm_start.py needs a HIP device (no CPU timing stands in for a GPU measurement)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    say(f"# tools/bench_warm_start.py --rounds {args.rounds} --reps {args.reps} on one {torch.cuda.get_device_name(0)} (gfx950)")
    out = {"device": torch.cuda.get_device_name(0), "kernel": kernel_section(dev, args.rounds, say)}
    out["pair_384x512_it12"] = pair_section(dev, 384, 512, 12, args.rounds, args.reps, have_scipy, say)
    out["pair_544x960_it32"] = pair_section(dev, 544, 960, 32, args.rounds, max(args.reps // 2, 1), have_scipy, say)
    torch.cuda.synchronize()
    if args.bench_parent:
        out["bench"] = bench_section(os.path.abspath(args.bench_parent), 3, say)
    say(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
