"""The on-the-fly correlation (AlternateCorrBlock, csrc/corr_alt.hip) against the materialised pyramid (CorrBlock).

    python tools/bench_alt_corr.py kernels     per-launch kernel times (kernel-timestamp events bound to the dispatch, what
                                               rocprofv3 --kernel-trace reports) of ff_corr_alt_prepare / ff_corr_alt_lookup
                                               beside ff_corr_build / ff_corr_lookup_tiled_fwd, and their rooflines
    python tools/bench_alt_corr.py forward     whole-forward pairs/s, alternate_corr True vs False, same process, alternating
                                               (captured forwards, GraphedForward)
    python tools/bench_alt_corr.py highres     ms per pair and max_memory_allocated at 1088x1920 and 2160x3840, 12 iterations
    python tools/bench_alt_corr.py --train     recorded passes (trained encoders): the training step (forward + backward,
                                               12 iterations, 8x368x496) on the on-the-fly route - forced by lowering
                                               corr_block._MAX_PYRAMID_BYTES - against the materialised one, alternating in
                                               one process; the backward kernel's time per pass (ff_corr_alt_lookup_bwd); one
                                               recorded 1088x1920 step under FF_CONV_PRECISION=fp32, time and max_memory_allocated

Roofline: a query needs 4 x 100 dot products of 256 channels = 102 400 MACs.  The split precisions issue them as three f16
MFMA products each (2.5 PFLOP/s dense f16), the exact-fp32 one as 32x32x2 fp32 MFMAs (157 TFLOP/s).  Minimal bytes of a
lookup: fmap1 and the four operand levels read once (1 KB per row), coordinates, and the 324 outputs written once.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from focusflow_official_amd import ops  # noqa: E402
from focusflow_official_amd.corr_block import AlternateCorrBlock, CorrBlock  # noqa: E402

DEV = "cuda:0"
F16_PEAK, F32_PEAK, HBM = 2.5e15, 157.3e12, 8.0e12


def _timed(which, fn, reps):
    ops.launch_timing_begin(which)
    for _ in range(reps):
        fn()
    n, tot, lo, hi = ops.launch_timing_end(which)
    return tot / max(n, 1), lo, n


def kernels(reps):
    print("per-launch kernel times (us): mean / min over", reps, "launches; CorrBlock = the materialised fp32 pyramid")
    for b, h, w in ((8, 48, 64), (1, 68, 120)):
        q = b * h * w
        g = torch.Generator().manual_seed(0)
        f1 = torch.randn(b, h, w, 256, generator=g).to(DEV)
        f2 = torch.randn(b, h, w, 256, generator=g).to(DEV)
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        base = torch.stack([xs, ys], -1).float()[None].repeat(b, 1, 1, 1)
        # a smooth flow (+-3 px across the image) plus sub-pixel noise: what the update loop's lookups see
        coords = (base + 3 * torch.sin(base / 9) + torch.rand(base.shape, generator=g) * 0.5).to(DEV).contiguous()
        with torch.no_grad():
            for prec in ("f16x3", "fp32"):
                ops.set_conv_precision(prec)
                alt = AlternateCorrBlock(f1, f2)
                alt(coords)
                prep, prep_lo, _ = _timed(ops.TIME_ALT_PREPARE, lambda: AlternateCorrBlock(f1, f2), reps)
                look, look_lo, _ = _timed(ops.TIME_ALT_LOOKUP, lambda: alt(coords), reps)
                macs = q * 102400.0
                t_mfma = macs * 2 * (3 if prec != "fp32" else 1) / (F16_PEAK if prec != "fp32" else F32_PEAK)
                rows = sum(b * (h >> l) * (w >> l) for l in range(4)) + q
                t_mem = (rows * 1024 + q * 8 + q * 324 * 4) / HBM
                bound = "matrix pipe" if t_mfma > t_mem else "memory"
                print(f"  {b}x{h}x{w} {prec:5s} alt prepare {prep:8.1f} (min {prep_lo:.1f})  alt lookup {look:8.1f} (min {look_lo:.1f})"
                      f"  | roofline lookup: MFMA {t_mfma * 1e6:.1f} us, bytes {t_mem * 1e6:.1f} us -> {bound}-bound,"
                      f" at {max(t_mfma, t_mem) * 1e6 / look * 100:.0f} % of it")
            ops.set_conv_precision("f16x3")
            cb = CorrBlock(f1, f2, pyramid_dtype="fp32")
            cb(coords)
            build, build_lo, _ = _timed(ops.TIME_CORR_BUILD, lambda: CorrBlock(f1, f2, pyramid_dtype="fp32"), reps)
            look, look_lo, _ = _timed(ops.TIME_LOOKUP, lambda: cb(coords), reps)
            print(f"  {b}x{h}x{w} f16x3 CorrBlock build {build:8.1f} (min {build_lo:.1f})  tiled lookup {look:8.1f} (min {look_lo:.1f})")
        del f1, f2, alt, cb
        torch.cuda.empty_cache()


def _model(alt):
    import json
    from argparse import Namespace
    from focusflow_official_amd import FF_RAFT_FUSION
    from oracle.weights import det_tensor
    cfg = Namespace(TRAIN=Namespace(MASK_CHANNEL=3, MASK_MODAL="point"), MODEL=Namespace(FUSION_TYPE="1x1conv", LOAD_MODULE_TO_BRANCH=False))
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_spec.json")) as f:
        sd = {k: det_tensor(k, s) for k, s, _ in json.load(f)}
    m = FF_RAFT_FUSION(use_fusion="parallel", fusion_channels=256, fuse_cnet=True, cfg=cfg, alternate_corr=alt)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def _inputs(b, h, w):
    from oracle import ffraft_ref as orc
    return [t.to(DEV) for t in orc.shifted_pair(b, h, w, seed=3)]


def forward(rounds, reps):
    from focusflow_official_amd.graph import GraphedForward
    for b, h, w, iters in ((8, 384, 512, 12), (1, 544, 960, 32)):
        inp = _inputs(b, h, w)
        gfs = {alt: GraphedForward(_model(alt), inp, raft_iters=iters) for alt in (False, True)}
        per = {False: [], True: []}
        for _ in range(rounds):
            for alt in (False, True):
                gf = gfs[alt]
                gf(*inp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    gf(*inp)
                torch.cuda.synchronize()
                per[alt].append(b * reps / (time.perf_counter() - t0))
        med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
        print(f"  {b}x{h}x{w} it{iters}: pairs/s materialised {med[False]:.1f}, alternate {med[True]:.1f}, ratio {med[True] / med[False]:.3f}"
              f"  (median of {rounds} alternating rounds of {reps} replays; all: {[round(x, 1) for x in per[False]]} / {[round(x, 1) for x in per[True]]})")
        del gfs
        torch.cuda.empty_cache()


def _train_step(m, inp, iters, w):
    for p in m.parameters():
        p.grad = None
    preds = m(*inp, raft_iters=iters)
    sum((p * x).sum() for p, x in zip(preds, w)).backward()


def train(rounds, reps):
    import warnings
    from focusflow_official_amd import corr_block
    warnings.simplefilter("ignore")
    default = corr_block._MAX_PYRAMID_BYTES
    b, h, w, iters = 8, 368, 496, 12
    m = _model(True).train()
    inp = _inputs(b, h, w)
    g = torch.Generator().manual_seed(5)
    wts = [(torch.randn(b, 2, h, w, generator=g) * 1e-3).to(DEV) for _ in range(iters)]
    per = {"materialised": [], "on-the-fly": []}
    for _ in range(rounds):
        for route in per:
            corr_block._MAX_PYRAMID_BYTES = default if route == "materialised" else 1
            _train_step(m, inp, iters, wts)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                _train_step(m, inp, iters, wts)
            torch.cuda.synchronize()
            per[route].append((time.perf_counter() - t0) * 1e3 / reps)
    med = {k: sorted(v)[len(v) // 2] for k, v in per.items()}
    print(f"  {b}x{h}x{w} it{iters} recorded step (fwd + bwd, fused update-loop node): materialised {med['materialised']:.2f} ms, "
          f"on-the-fly {med['on-the-fly']:.2f} ms, ratio {med['on-the-fly'] / med['materialised']:.3f}  (median of {rounds} "
          f"alternating rounds of {reps} steps; all: {[round(x, 2) for x in per['materialised']]} / {[round(x, 2) for x in per['on-the-fly']]})")
    corr_block._MAX_PYRAMID_BYTES = 1
    ops.launch_timing_begin(ops.TIME_ALT_LOOKUP_BWD)
    for _ in range(reps):
        _train_step(m, inp, iters, wts)
    n, tot, lo, hi = ops.launch_timing_end(ops.TIME_ALT_LOOKUP_BWD)
    print(f"  {b}x{h}x{w} it{iters} ff_corr_alt_lookup_bwd main kernel: {tot / max(n, 1):.1f} us per pass (min {lo:.1f}, max {hi:.1f}, "
          f"{n} launches)")
    corr_block._MAX_PYRAMID_BYTES = default
    del m, inp, wts
    torch.cuda.empty_cache()
    # one recorded 1088x1920 pair in fp32 (its materialised pyramid, 5.7 GB, is beyond the lookup's resource: the on-the-fly
    # route is selected by the size itself)
    ops.set_conv_precision("fp32")
    m = _model(True).train()
    inp = _inputs(1, 1088, 1920)
    wts = [(torch.randn(1, 2, 1088, 1920, generator=g) * 1e-3).to(DEV) for _ in range(iters)]
    _train_step(m, inp, iters, wts)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    nrep = max(1, reps // 4)
    for _ in range(nrep):
        _train_step(m, inp, iters, wts)
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    print(f"  1x1088x1920 it{iters} recorded step FF_CONV_PRECISION=fp32 alternate_corr=True: "
          f"{(time.perf_counter() - t0) * 1e3 / nrep:.1f} ms, max_memory_allocated {torch.cuda.max_memory_allocated() / 1e9:.2f} GB, "
          f"gradients finite: {finite}")
    ops.set_conv_precision("f16x3")


def highres(reps, precision):
    ops.set_conv_precision(precision)
    m = _model(True)
    for h, w in ((1088, 1920), (2160, 3840)):
        try:
            inp = _inputs(1, h, w)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            with torch.no_grad():
                lo, _ = m(*inp, raft_iters=12, test_mode=True)
                finite = bool(torch.isfinite(lo).all())
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    m(*inp, raft_iters=12, test_mode=True)
                torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / reps
            print(f"  1x{h}x{w} it12 alternate_corr=True FF_CONV_PRECISION={precision}: {ms:.1f} ms per pair, "
                  f"max_memory_allocated {torch.cuda.max_memory_allocated() / 1e9:.2f} GB, flow finite: {finite}")
        except Exception as e:       # (report which kernel refuses the shape, and go on)
            print(f"  1x{h}x{w} it12 alternate_corr=True: refused: {type(e).__name__}: {e}")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", choices=("kernels", "forward", "highres", "train"))
    ap.add_argument("--train", action="store_true", help="the recorded-pass leg (= what 'train')")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="f16x3", help="FF_CONV_PRECISION of the highres leg")
    a = ap.parse_args()
    if a.train:
        a.what = "train"
    if a.what is None:
        ap.error("name a leg (kernels, forward, highres) or pass --train")
    print(f"{torch.cuda.get_device_name(0)}  bench_alt_corr {a.what}")
    {"kernels": lambda: kernels(a.reps), "forward": lambda: forward(a.rounds, a.reps), "highres": lambda: highres(max(1, a.reps // 10), a.precision),
     "train": lambda: train(a.rounds, max(2, a.reps // 2))}[a.what]()
