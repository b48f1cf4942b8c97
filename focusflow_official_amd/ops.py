"""Tensor-level wrappers over the C ABI (device pointers in, device pointers out).

Activations are NHWC fp32 torch tensors of shape (B, H, W, C) whose last dim is
contiguous; a tensor may be a channel slice of a wider buffer (stride(2) = ld).
torch is used for allocation and stream handles only — all arithmetic happens
in libfocusflow_hip.so.
"""
import contextlib
import ctypes as C
import math
import os
import threading
from typing import List, Optional, Sequence

import torch

from . import _hip
from ._hip import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, FFConvParams  # noqa: F401

Tensor = torch.Tensor


# The current stream of the current device as a raw hipStream_t.  torch.cuda.current_stream() builds a Stream object through
# several Python layers (~8 us; a one-pair forward asks ~350 times and is host-bound): the two C entry points behind it
# are used directly where this torch has them.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    if _raw_stream is not None and _raw_device is not None:
        return C.c_void_p(_raw_stream(_raw_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Arithmetic of the forward convolutions / correlation volume:
#   "f16x3" (default) fp16-split operands, 3 f16 MFMAs: fp32-level accuracy (see csrc/conv_split.hip)
#   "fp32"  exact fp32 MFMA            "f16"  plain fp16 operands (reduced precision, throughput mode)
_PRECISIONS = {"fp32": _hip.W_F32, "f16x3": _hip.W_F16X3, "f16": _hip.W_F16}
_conv_precision = os.environ.get("FF_CONV_PRECISION", "f16x3")


def set_conv_precision(name: str):
    global _conv_precision
    if name not in _PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}")
    _conv_precision = name


def conv_precision() -> str:
    return _conv_precision


def w_format() -> int:
    return _PRECISIONS[_conv_precision]


def pack_split(rows_f32: Tensor) -> Tensor:
    """fp32 [rows][K] -> split fp16 rows (uint8 view [rows][ceil(K/32)*128])."""
    _require_gpu(rows_f32)
    rows, k = rows_f32.shape
    assert rows_f32.is_contiguous()
    dst = torch.empty((rows, (k + 31) // 32 * 128), dtype=torch.uint8, device=rows_f32.device)
    _hip.call("ff_pack_split_f16", _p(rows_f32), _p(dst), rows, k, _stream())
    return dst


def pack_frag16(w_split: Tensor, rows: int) -> Tensor:
    """Split rows (pack_split) -> MFMA-fragment order (ff_pack_frag16) for FFConvParams.w_frag."""
    nkc = w_split.shape[1] // 128
    dst = torch.empty(((rows + 15) // 16) * nkc * 2048, dtype=torch.uint8, device=w_split.device)
    _hip.call("ff_pack_frag16", _p(w_split), _p(dst), rows, nkc, _stream())
    return dst


class _StreamPolicy(threading.local):
    """Per-THREAD stream policy of the forward passes (two models driven from two threads do not see each other's).
    single_stream: set by a caller that brackets single launches with events (bench.py's roofline_conv leg) - every
    forward then runs on ONE stream, so that the bracketed durations add up to wall time instead of overlapping.
    encoder_streams_ok: set per forward by RAFT._forward - below ~3.5 pairs of 384x512 a step is host-bound and the
    fork / join events of the encoder streams cost more than the overlap gains (configs[4] at one pair: 16.4 -> 16.7 ms)."""
    single_stream = False
    encoder_streams_ok = True


policy = _StreamPolicy()

# Optional per-launch timing of ONE entry point with HIP events recorded on the
# launch stream (bench.py's roofline leg).  Off unless profile_begin() is called.
_prof_on = False
_prof_events = {}
_prof_notes = {}      # label -> per-launch annotation (conv: useful FLOP of the launch)


def profile_begin(*labels: str):
    """Time every launch carrying one of `labels` with a HIP event pair on the launch stream."""
    global _prof_on
    _prof_on = True
    _prof_events.clear()
    _prof_notes.clear()
    for lb in labels:
        _prof_events[lb] = []
        _prof_notes[lb] = []


def profile_end():
    """-> {label: [per-launch milliseconds]} (synchronises)."""
    global _prof_on
    _prof_on = False
    torch.cuda.synchronize()
    out = {lb: [a.elapsed_time(b) for a, b in ev] for lb, ev in _prof_events.items()}
    _prof_events.clear()
    return out


def profile_notes(label):
    """Annotations recorded next to the timings of `label` (read before the next profile_begin)."""
    return list(_prof_notes.get(label, []))


TIME_LOOKUP, TIME_CORR_BUILD, TIME_PROBE = 1, 2, 3          # include/focusflow_hip.h: FF_TIME_*


def probe_memory_kernel(src: Tensor, dst: Tensor, seg_bytes: int, blocks: int, trips: int, salt: int):
    """ff_probe_memory_kernel: the memory-only companion of the lookup (measurement aid) -> (bytes read, bytes written)."""
    if not (src.is_cuda and dst.is_cuda):
        raise _hip.FocusFlowHipError("ff_probe_memory_kernel: device buffers only")
    rd, wr = C.c_longlong(0), C.c_longlong(0)
    _hip.call("ff_probe_memory_kernel", _p(src), src.numel() * src.element_size(), _p(dst), dst.numel() * dst.element_size(), seg_bytes,
              blocks, trips, salt, C.byref(rd), C.byref(wr), _stream())
    return rd.value, wr.value


def launch_timing_begin(*which: int):
    """Kernel-timestamp timing of the library's lookup / corr-build launches (ff_launch_timing_begin): HIP events bound
    to the dispatch itself, on whatever stream the launch goes to."""
    for w in which:
        _hip.call("ff_launch_timing_begin", w)


def launch_timing_end(which: int):
    """-> (launches, total_us, min_us, max_us) since launch_timing_begin; waits for the launches."""
    n, tot, lo, hi = C.c_longlong(0), C.c_double(0), C.c_double(0), C.c_double(0)
    _hip.call("ff_launch_timing_end", which, C.byref(n), C.byref(tot), C.byref(lo), C.byref(hi))
    return n.value, tot.value, lo.value, hi.value


def _timed_call(label, name, *args, note=None):
    if _prof_on and label in _prof_events:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _hip.call(name, *args)
        b.record()
        _prof_events[label].append((a, b))
        _prof_notes[label].append(note)
    else:
        _hip.call(name, *args)


def _require_gpu(t: Tensor):
    if not t.is_cuda:
        raise _hip.FocusFlowHipError(
            "the FF-RAFT hot path runs on a HIP device only (got a CPU tensor); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise _hip.FocusFlowHipError(f"fp32 tensors expected, got {t.dtype}")


def _ld(t: Tensor) -> int:
    """floats per pixel of an NHWC (B,H,W,C) view; checks it is pixel-dense."""
    _require_gpu(t)
    b, h, w, c = t.shape
    ld = t.stride(2) if w > 1 else (t.stride(1) if h > 1 else max(t.stride(0), c))
    if t.stride(3) != 1 or (w > 1 and h > 1 and t.stride(1) != w * ld) or (b > 1 and t.stride(0) != h * w * ld):
        raise _hip.FocusFlowHipError(f"not an NHWC view: shape {tuple(t.shape)} strides {t.stride()}")
    return ld


def _p(t: Optional[Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def empty_nhwc(b, h, w, c, like: Tensor) -> Tensor:
    return torch.empty((b, h, w, c), dtype=torch.float32, device=like.device)


class SplitT:
    """An NHWC activation in the split-pair format (FF_FMT_SPLIT, include/focusflow_hip.h): shape, strides and bytes of its
    fp32 form, but every 32-channel chunk of a pixel holds [x0: 32 fp16 | x1: 32 fp16] - what a convolution loader makes
    of the fp32 values, written by the producer so that the consumer's patch goes L2 -> LDS by LDS-DMA.  Only convolutions
    read it (ops.conv2d sets FFConvParams.x_fmt); `.t` is the raw storage and means nothing as floats."""
    __slots__ = ("t",)

    def __init__(self, t: Tensor):
        self.t = t

    @property
    def shape(self):
        return self.t.shape

    @property
    def device(self):
        return self.t.device

    def __getitem__(self, idx):
        r = self.t[idx]
        off = (r.data_ptr() - self.t.data_ptr()) // 4
        ld = _ld(self.t)
        if (off % ld) % 32 or r.shape[3] % 32:
            raise _hip.FocusFlowHipError("a split-pair tensor can only be sliced at multiples of 32 channels")
        return SplitT(r)

    def record_stream(self, s):
        self.t.record_stream(s)

    def float(self) -> Tensor:
        """Back to fp32 ((x0 + x1) / 4: 22 significant bits) - tests and debugging."""
        return split_copy(self.t, to_split=False)


def _raw(x):
    return x.t if isinstance(x, SplitT) else x


def split_copy(x: Tensor, act: int = ACT_NONE, to_split: bool = True, out: Optional[Tensor] = None):
    """fp32 NHWC -> SplitT (ff_split_copy; an activation on the way), or - to_split=False - the raw storage of a SplitT back
    to fp32."""
    b, h, w, c = x.shape
    if out is None:
        out = empty_nhwc(b, h, w, c, x)
    _hip.call("ff_split_copy", _p(x), _ld(x), _p(out), _ld(out), b * h * w, c, act, 1 if to_split else 0, _stream())
    return SplitT(out) if to_split else out


# ----------------------------------------------------------------------------
def pack_conv_weight(w_oihw: Tensor, dst: Tensor, cin_pad: int, cout_offset: int = 0):
    """OIHW parameter -> rows [cout_offset, cout_offset+Cout) of dst [rows][KH*KW*cin_pad]."""
    _require_gpu(w_oihw)
    co, ci, kh, kw = w_oihw.shape
    assert dst.is_contiguous() and dst.shape[1] == kh * kw * cin_pad and dst.shape[0] >= cout_offset + co
    _hip.call("ff_pack_conv_weight", _p(w_oihw.contiguous()), co, ci, kh, kw, _p(dst), cin_pad, cout_offset, _stream())


def conv2d(xs: Sequence[Tensor], wpack: Tensor, bias: Optional[Tensor], cout: int, kh: int, kw: int,
           stride: int = 1, pad=(0, 0), act: int = ACT_NONE, out: Optional[Tensor] = None,
           res: Optional[Tensor] = None, act_res: int = ACT_NONE, ch_scale: Optional[Tensor] = None,
           ch_shift: Optional[Tensor] = None, out_scale: float = 1.0, w_fmt: int = 0, dilation: int = 1,
           x_amax: Optional[Tensor] = None, in_scale: Optional[Tensor] = None, in_shift: Optional[Tensor] = None,
           in_act: int = ACT_NONE, res2: Optional[Tensor] = None, res_split: int = 0,
           ep_rh: Optional[Tensor] = None, ep_split: int = 0, ep_blend=None, want_stats: bool = False, ep_coords=None,
           y_split=False, y2_split: bool = False, ep_motion_tail: Optional[Tensor] = None, w_frag: Optional[Tensor] = None):
    """Convolution over the channel-concatenation of `xs` (see FFConvParams).  want_stats: -> (out, stats) with the
    per-sample {sum, sum of squares} table of the output (what norm_stats(out, True) returns): from the convolution's own
    epilogue where the kernel can (FFConvParams.stats_part), else from a norm_stats pass.  res2 / res_split: output channels
    >= res_split take their residual from `res2` (paired 1x1 fusion convs).  `wpack` is fp32
    [Cout][K] (w_fmt 0) or the split rows of pack_split (w_fmt 1/2).  x_amax: device word holding the bits of
    max|x| (act_bwd): the split formats then scale the input by a power of two so that gradients fit fp16."""
    if isinstance(pad, int):
        pad = (pad, pad)
    fmts = [1 if isinstance(x, SplitT) else 0 for x in xs]
    xs = [_raw(x) for x in xs]
    x0 = xs[0]
    b, h, w, _ = x0.shape
    ho = (h + 2 * pad[0] - dilation * (kh - 1) - 1) // stride + 1
    wo = (w + 2 * pad[1] - dilation * (kw - 1) - 1) // stride + 1
    if out is None:
        if y_split is not False:      # a split-pair chunk is 32 channels: the buffer holds Cout rounded up to 32 (the x1 half of the last chunk)
            full = empty_nhwc(b, ho, wo, (cout + 31) // 32 * 32, x0)
            out = full if full.shape[3] == cout else full[..., :cout]
        else:
            out = empty_nhwc(b, ho, wo, (cout + 3) // 4 * 4, x0)[..., :cout] if cout % 4 else empty_nhwc(b, ho, wo, cout, x0)
    p = FFConvParams()
    cin = 0
    for i, x in enumerate(xs):
        assert x.shape[:3] == x0.shape[:3]
        p.x[i] = x.data_ptr()
        p.x_ld[i] = _ld(x)
        p.x_c[i] = x.shape[3]
        p.x_gstride[i] = 0
        p.x_fmt[i] = fmts[i]
        cin += x.shape[3]
    kdim = kh * kw * cin if w_fmt == 0 else (kh * kw * cin + 31) // 32 * 128
    assert wpack.is_contiguous() and wpack.shape[-1] == kdim and wpack.shape[0] >= cout, \
        f"packed weight {tuple(wpack.shape)} vs Cout {cout}, K {kh * kw * cin} (format {w_fmt})"
    p.groups, p.B, p.H, p.W = 1, b, h, w
    p.w, p.w_gstride = wpack.data_ptr(), 0
    if w_frag is not None:      # the same weights in fragment order (pack_frag16): read by conv_dma.hip only
        p.w_frag = w_frag.data_ptr()
    p.bias = bias.data_ptr() if bias is not None else None
    p.ch_scale = ch_scale.data_ptr() if ch_scale is not None else None
    p.ch_shift = ch_shift.data_ptr() if ch_shift is not None else None
    p.out_scale = out_scale
    p.res = res.data_ptr() if res is not None else None
    p.res_ld = _ld(res) if res is not None else 0
    if res2 is not None:
        p.res2, p.res2_ld, p.res_split = res2.data_ptr(), _ld(res2), res_split
    if ep_rh is not None:       # FF_EP_GRU_RH: output channels >= ep_split leave multiplied by ep_rh (the z|r conv writes [z | r*h])
        p.ep_mode, p.ep_split, p.ep_a, p.ep_a_ld = 1, ep_split, ep_rh.data_ptr(), _ld(ep_rh)
    elif ep_coords is not None:  # FF_EP_COORDS: (coords1, flow4) - the flow head also takes the coordinate step
        c1, f4 = ep_coords
        assert c1.is_contiguous() and c1.shape == (b, ho, wo, 2) and f4.is_contiguous() and f4.shape == (b, ho, wo, 4)
        p.ep_mode, p.ep_a, p.ep_b = 3, c1.data_ptr(), f4.data_ptr()
    elif ep_blend is not None:  # FF_EP_GRU_BLEND: (z, h) -> the output is (1 - z) h + z v (the q conv writes the new state)
        z, hprev = ep_blend
        p.ep_mode, p.ep_a, p.ep_a_ld, p.ep_b, p.ep_b_ld = 2, z.data_ptr(), _ld(z), hprev.data_ptr(), _ld(hprev)
    elif ep_motion_tail is not None:   # FF_EP_MOTION_TAIL: channels Cout, Cout + 1 of the padded output = coords1 - pixel grid
        assert ep_motion_tail.is_contiguous() and ep_motion_tail.shape == (b, ho, wo, 2)
        p.ep_mode, p.ep_a = 4, ep_motion_tail.data_ptr()
    p.y, p.y_ld, p.y_gstride = out.data_ptr(), _ld(out), 0
    if y_split is not False:
        p.y_fmt, p.y_fmt_from = 1, (0 if y_split is True else int(y_split))
    out2 = None
    if y2_split:
        out2 = empty_nhwc(b, ho, wo, (cout + 31) // 32 * 32, x0)
        p.y2, p.y2_ld = out2.data_ptr(), _ld(out2)
    p.Ho, p.Wo, p.Cout = ho, wo, cout
    p.KH, p.KW, p.stride, p.pad_h, p.pad_w = kh, kw, stride, pad[0], pad[1]
    p.act, p.act_res, p.w_format = act, act_res, w_fmt
    p.dil_h = p.dil_w = dilation
    p.x_amax = x_amax.data_ptr() if x_amax is not None else None
    if in_scale is not None:   # norm_coeffs tables [B][Cin]: the input is read as in_act(x * scale + shift) (normalise-on-load)
        assert in_scale.shape == in_shift.shape == (b, cin) and in_scale.is_contiguous() and in_shift.is_contiguous()
        p.in_scale, p.in_shift, p.in_act = in_scale.data_ptr(), in_shift.data_ptr(), in_act
    assert out.shape[:3] == (b, ho, wo) and out.shape[3] >= cout
    if _range_word is not None and w_fmt and x_amax is None and in_scale is None:
        for x, f in zip(xs, fmts):
            if not f:          # (a split-pair tensor was range-checked as the fp32 values its producer held)
                _range_probe(x)
    klen = cin * kh * kw
    plain = not any(fmts) and y_split is False and not y2_split                # (the split-pair kernels have no K splits)
    if plain and w_fmt and not p.ep_mode and b * ho * wo <= 16384 and klen > 1152:       # small plane, long reduction: ask the library whether K splits pay
        # reductions of 36-72 tap steps are split only when no host time is at stake: while a hipGraph is being captured
        short = klen <= 2304
        if not short or torch.cuda.is_current_stream_capturing():
            p.splitk = -1 if short else 0
            nsplit = _hip.load().ff_conv2d_splitk_hint(C.byref(p))
            p.splitk = 0
            if nsplit > 1:
                ws = torch.empty(nsplit * b * ho * wo * cout, dtype=torch.float32, device=x0.device)
                p.splitk_ws, p.splitk = ws.data_ptr(), nsplit
    nparts = _hip.load().ff_conv2d_stats_parts(C.byref(p)) if want_stats and CONV_STATS and not p.splitk else 0
    if nparts:
        parts = torch.empty(b * nparts * cout * 4, dtype=torch.float32, device=x0.device)
        p.stats_part = parts.data_ptr()
        _timed_call("conv", "ff_conv2d_fwd", C.byref(p), _stream(), note=(2.0 * b * ho * wo * cout * kh * kw * cin, w_fmt))
        stats = _zero_stats(b, cout, x0.device)
        _hip.call("ff_norm_stats_finish", _p(parts), b, nparts, cout, _p(stats), _stream())
        return out, stats
    _timed_call("conv", "ff_conv2d_fwd", C.byref(p), _stream(), note=(2.0 * b * ho * wo * cout * kh * kw * cin, w_fmt))
    if want_stats:
        return out, norm_stats(out, per_sample=True)
    if y_split is True:
        out = SplitT(out)
    if y2_split:
        return out, SplitT(out2)
    return out


class TiledPyramid:
    """The 4-level correlation pyramid in the tiled HBM layout of csrc/corr_layout.h.

    levels[l]: (B*Q, plane_l) tensor, float32 or float16; a plane is a grid of 128-byte tiles (8 x 4 floats or
    8 x 8 halfs) over the level's h_l x w_l values.  `rowmajor(l)` converts a level back to (B*Q, h_l, w_l) fp32
    (tests / debugging only)."""

    def __init__(self, levels: List[Tensor], h0: int, w0: int, half: bool):
        self.levels, self.h0, self.w0, self.half = levels, h0, w0, half

    @staticmethod
    def plane_elems(h0: int, w0: int, level: int, half: bool) -> int:
        n = _hip.load().ff_corr_plane_elems(h0, w0, level, int(half))
        if n <= 0:
            raise _hip.FocusFlowHipError(f"ff_corr_plane_elems({h0}, {w0}, {level}) failed")
        return n

    @classmethod
    def empty(cls, planes: int, h0: int, w0: int, half: bool, device, zero: bool = False) -> "TiledPyramid":
        # ONE allocation for the four levels (each starts on a 256-byte boundary): the lookup kernel addresses them
        # through a single buffer resource (csrc/corr_lookup_dma.hip), which needs them within 4 GB of each other
        dt = torch.float16 if half else torch.float32
        mk = torch.zeros if zero else torch.empty
        esz = 2 if half else 4
        n = [planes * cls.plane_elems(h0, w0, l, half) for l in range(4)]
        start, total = [], 0
        for l in range(4):
            start.append(total)
            total += (n[l] * esz + 255) // 256 * 256 // esz
        flat = mk((total,), dtype=dt, device=device)
        return cls([flat[start[l]:start[l] + n[l]].view(planes, n[l] // planes) for l in range(4)], h0, w0, half)

    def ptrs(self):
        return (C.c_void_p * 4)(*[lv.data_ptr() for lv in self.levels])

    def rowmajor(self, level: int) -> Tensor:
        n = self.levels[level].shape[0]
        out = torch.empty((n, self.h0 >> level, self.w0 >> level), dtype=torch.float32, device=self.levels[level].device)
        _hip.call("ff_corr_retile", _p(out), _p(self.levels[level]), n, self.h0, self.w0, level, int(self.half), 0, _stream())
        return out

    @classmethod
    def from_rowmajor(cls, levels: List[Tensor], half: bool = False) -> "TiledPyramid":
        """(B*Q, h_l, w_l) fp32 planes -> tiled storage (fp16: rounded to nearest even); pads are zero."""
        n, h0, w0 = levels[0].shape
        pyr = cls.empty(n, h0, w0, half, levels[0].device, zero=True)
        for l, lv in enumerate(levels):
            assert lv.shape == (n, h0 >> l, w0 >> l) and lv.is_contiguous() and lv.dtype == torch.float32
            _hip.call("ff_corr_retile", _p(lv), _p(pyr.levels[l]), n, h0, w0, l, int(half), 1, _stream())
        return pyr


def corr_build(fmap1: Tensor, fmap2: Tensor, half: bool = False) -> TiledPyramid:
    """CorrBlock.__init__ (corr.py:12-27, :52-60) in one launch: all-pairs volume / sqrt(C) on the f16 matrix pipe with
    fp16-split operands, the three 2x2 average-pooling levels from the accumulators, everything written once in the
    tiled layout (fp32, or fp16 storage = BASELINE configs[4]).  The exact-fp32 MFMA precision goes through the
    grouped-conv volume + pooling pass and is re-tiled."""
    b, h, w, c = fmap1.shape
    q = h * w
    assert fmap1.is_contiguous() and fmap2.is_contiguous() and fmap2.shape == fmap1.shape
    _require_gpu(fmap1)
    if w_format() == _hip.W_F32 or c != 256:       # (the one-term f16 mode builds the volume with the three-term kernel too)
        return TiledPyramid.from_rowmajor(corr_pyramid(corr_volume(fmap1, fmap2), h, w), half)
    esz = fmap1.element_size()
    if fmap2.data_ptr() == fmap1.data_ptr() + b * q * c * esz and fmap1.untyped_storage().data_ptr() == fmap2.untyped_storage().data_ptr():
        # both frames went through fnet as one batch: split them with one launch
        both = torch.empty((2 * b * q, c * 4), dtype=torch.uint8, device=fmap1.device)
        _hip.call("ff_pack_split_f16", _p(fmap1), _p(both), 2 * b * q, c, _stream())
        f1s, f2s = both[:b * q], both[b * q:]
    else:
        f1s, f2s = pack_split(fmap1.view(b * q, c)), pack_split(fmap2.view(b * q, c))
    pyr = TiledPyramid.empty(b * q, h, w, half, fmap1.device)
    _timed_call("corr_volume", "ff_corr_build", _p(f1s), _p(f2s), pyr.ptrs(), b, h, w, c, int(half), _stream())
    return pyr


def corr_lookup_tiled(pyr: TiledPyramid, coords: Tensor, want_taps: bool = False, out: Optional[Tensor] = None):
    """CorrBlock.__call__ (corr.py:29-50) on a TiledPyramid.  coords: (B, H, W, 2) [x, y].  Returns (B, H, W, 324)
    (+ int32 taps (B*H*W, 4, 2, 9)).  `out`: a (B,H,W,324) view of a wider buffer."""
    _require_gpu(coords)
    b, h, w, _ = coords.shape
    assert coords.is_contiguous() and pyr.levels[0].shape[0] == b * h * w
    if out is None:
        out = empty_nhwc(b, h, w, 324, coords)
    assert out.shape == (b, h, w, 324)
    taps = torch.empty((b * h * w, 4, 2, 9), dtype=torch.int32, device=coords.device) if want_taps else None
    _timed_call("lookup", "ff_corr_lookup_tiled_fwd", pyr.ptrs(), int(pyr.half), _p(coords), b * h * w, pyr.h0, pyr.w0,
                _p(out), _ld(out), _p(taps), _stream())
    return (out, taps) if want_taps else out


class AltOperands:
    """What ff_corr_alt_prepare leaves for the on-the-fly lookup (AlternateCorrBlock): the operand rows of fmap1 and of the
    four levels of fmap2 (split pairs, or fp32 rows with levels 0 = fmap2 itself).  Memory linear in the image area."""
    __slots__ = ("f1", "levels", "split", "b", "h0", "w0", "_keep")

    def ptrs(self):
        return (C.c_void_p * 4)(*[lv.data_ptr() for lv in self.levels])


TIME_ALT_LOOKUP, TIME_ALT_PREPARE, TIME_ALT_LOOKUP_BWD = 4, 5, 6      # include/focusflow_hip.h: FF_TIME_*


def corr_alt_prepare(fmap1: Tensor, fmap2: Tensor) -> AltOperands:
    """AlternateCorrBlock.__init__: pooled levels 1-3 of fmap2 and the operand form of the lookup (ff_corr_alt_prepare), one
    launch.  The split precisions get fp16 split pairs of fmap1 and of every level; the exact-fp32 one fp32 rows of levels 1-3."""
    b, h, w, c = fmap1.shape
    _require_gpu(fmap1)
    _require_gpu(fmap2)
    assert fmap1.is_contiguous() and fmap2.is_contiguous() and fmap2.shape == fmap1.shape
    if c != 256:
        raise _hip.FocusFlowHipError(f"corr_alt_prepare: {c} feature channels (the kernels are built for 256)")
    split = w_format() != _hip.W_F32
    rows = [b * (h >> l) * (w >> l) for l in range(4)]
    first = 0 if split else 1
    flat = torch.empty((sum(rows[first:]) + (b * h * w if split else 0)) * 256, dtype=torch.float32, device=fmap1.device)
    views, o = [], 0
    for l in range(first, 4):
        views.append(flat[o * 256:(o + rows[l]) * 256].view(rows[l], 256))
        o += rows[l]
    levels = views if split else [fmap2.view(rows[0], 256)] + views
    f1 = flat[o * 256:].view(b * h * w, 256) if split else fmap1.view(b * h * w, 256)
    ops = AltOperands()
    ops.f1, ops.levels, ops.split, ops.b, ops.h0, ops.w0, ops._keep = f1, levels, split, b, h, w, (fmap1, fmap2, flat)
    lv = (C.c_void_p * 4)(*[(x.data_ptr() if (split or l > 0) else 0) for l, x in enumerate(levels)])
    _timed_call("corr_alt_prepare", "ff_corr_alt_prepare", _p(fmap1), _p(fmap2), b, h, w, c, int(split), _p(f1) if split else C.c_void_p(0),
                lv, _stream())
    return ops


def corr_alt_lookup(ops: AltOperands, coords: Tensor, want_taps: bool = False, out: Optional[Tensor] = None):
    """AlternateCorrBlock.__call__ (ff_corr_alt_lookup): coords (B, H, W, 2) [x, y] -> (B, H, W, 324) (+ int32 taps
    (B*H*W, 4, 2, 9), bit-identical to corr_lookup_tiled's).  `out`: a (B,H,W,324) view of a wider buffer."""
    _require_gpu(coords)
    b, h, w, _ = coords.shape
    assert coords.is_contiguous() and (b, h, w) == (ops.b, ops.h0, ops.w0)
    if out is None:
        out = empty_nhwc(b, h, w, 324, coords)
    assert out.shape == (b, h, w, 324)
    taps = torch.empty((b * h * w, 4, 2, 9), dtype=torch.int32, device=coords.device) if want_taps else None
    _timed_call("lookup", "ff_corr_alt_lookup", _p(ops.f1), ops.ptrs(), int(ops.split), _p(coords), b, h, w, _p(out), _ld(out),
                _p(taps), _stream())
    return (out, taps) if want_taps else out


def corr_alt_lookup_bwd(ops: AltOperands, coords_list: List[Tensor], dout_list: List[Optional[Tensor]]):
    """Backward of the on-the-fly lookups of one recorded pass (ff_corr_alt_lookup_bwd, one launch per 32 lookups + a fold):
    coords_list[t] (B, H, W, 2) as the forward's lookup t saw them, dout_list[t] (B, H, W, 324) - or a (B, H, W, 324) view of
    a wider NHWC buffer, or None (no gradient reached that lookup) -> (d fmap1, d fmap2), NHWC (B, H, W, 256).  Exact fp32
    arithmetic in every precision: the split precisions get fp32 rows of levels 1-3 for the duration of the call."""
    fmap1, fmap2 = ops._keep[0], ops._keep[1]
    b, h, w = ops.b, ops.h0, ops.w0
    pairs = [(c, d) for c, d in zip(coords_list, dout_list) if d is not None]
    df1 = torch.empty((b, h, w, 256), dtype=torch.float32, device=fmap1.device)
    if not pairs:
        return df1.zero_(), torch.zeros_like(df1)
    for c, d in pairs:
        _require_gpu(c)
        assert c.is_contiguous() and tuple(c.shape) == (b, h, w, 2) and tuple(d.shape) == (b, h, w, 324)
    ld = {_ld(d) for _, d in pairs}
    if len(ld) != 1:
        pairs = [(c, d.contiguous()) for c, d in pairs]
        ld = {324}
    rows = [b * (h >> l) * (w >> l) for l in range(4)]
    if ops.split:      # fp32 rows of levels 1-3 (ff_corr_alt_prepare with split == 0)
        flat = torch.empty(sum(rows[1:]) * 256, dtype=torch.float32, device=fmap1.device)
        lv32, o = [fmap2.view(rows[0], 256)], 0
        for l in range(1, 4):
            lv32.append(flat[o * 256:(o + rows[l]) * 256].view(rows[l], 256))
            o += rows[l]
        lv = (C.c_void_p * 4)(0, *[x.data_ptr() for x in lv32[1:]])
        _hip.call("ff_corr_alt_prepare", _p(fmap1), _p(fmap2), b, h, w, 256, 0, C.c_void_p(0), lv, _stream())
    else:
        lv32 = ops.levels
    df2 = torch.zeros((b, h, w, 256), dtype=torch.float32, device=fmap1.device)
    scratch = torch.zeros(sum(rows[1:]) * 256, dtype=torch.float32, device=fmap1.device)
    dl, o = [df2], 0
    for l in range(1, 4):
        dl.append(scratch[o * 256:(o + rows[l]) * 256])
        o += rows[l]
    n = len(pairs)
    cl = (C.c_void_p * n)(*[c.data_ptr() for c, _ in pairs])
    gl = (C.c_void_p * n)(*[d.data_ptr() for _, d in pairs])
    _timed_call("corr_alt_lookup_bwd", "ff_corr_alt_lookup_bwd", _p(fmap1), (C.c_void_p * 4)(*[x.data_ptr() for x in lv32]), cl, gl, n,
                ld.pop(), b, h, w, _p(df1), (C.c_void_p * 4)(*[x.data_ptr() for x in dl]), _stream())
    return df1, df2


def corr_volume(fmap1: Tensor, fmap2: Tensor) -> Tensor:
    """corr.py:52-60: vol[b][i][j] = <f1[b,i,:], f2[b,j,:]> / sqrt(C) as a grouped 1x1 conv
    whose per-sample weights are fmap2.  Returns (B, Q, Q) planes [B*Q][H8][W8]."""
    b, h, w, c = fmap1.shape
    q = h * w
    assert fmap1.is_contiguous() and fmap2.is_contiguous() and fmap2.shape == fmap1.shape
    vol = torch.empty((b, q, q), dtype=torch.float32, device=fmap1.device)
    p = FFConvParams()
    p.x[0], p.x_ld[0], p.x_c[0], p.x_gstride[0] = fmap1.data_ptr(), c, c, q * c
    p.groups, p.B, p.H, p.W = b, 1, h, w
    p.w_format = w_format()
    if p.w_format == 0:
        p.w, p.w_gstride = fmap2.data_ptr(), q * c
    else:  # fmap2 plays the weights: split it once per pair
        f2s = pack_split(fmap2.view(b * q, c))
        p.w, p.w_gstride = f2s.data_ptr(), q * f2s.shape[1] // 4
    p.out_scale = 1.0 / math.sqrt(c)
    p.y, p.y_ld, p.y_gstride = vol.data_ptr(), q, q * q
    p.Ho, p.Wo, p.Cout = h, w, q
    p.KH = p.KW = p.stride = 1
    _require_gpu(fmap1)
    _timed_call("corr_volume", "ff_conv2d_fwd", C.byref(p), _stream())
    return vol


def corr_pyramid(vol: Tensor, h: int, w: int) -> List[Tensor]:
    b, q, _ = vol.shape
    n = b * q
    lv = [vol.view(n, h, w)]
    hh, ww = h, w
    for _ in range(3):
        hh, ww = hh // 2, ww // 2
        lv.append(torch.empty((n, hh, ww), dtype=torch.float32, device=vol.device))
    _hip.call("ff_corr_pyramid", _p(lv[0]), _p(lv[1]), _p(lv[2]), _p(lv[3]), n, h, w, _stream())
    return lv


def corr_lookup(levels: List[Tensor], coords: Tensor, radius: int = 4, want_taps: bool = False,
                out: Optional[Tensor] = None):
    """coords: (B, H, W, 2) [x, y].  Returns (B, H, W, L*(2r+1)^2) (+ int32 taps).  `out`: a (B,H,W,nk) view of a
    wider buffer (the caller owns the channels beyond nk)."""
    _require_gpu(coords)
    b, h, w, _ = coords.shape
    assert coords.is_contiguous()
    nl = len(levels)
    nk = nl * (2 * radius + 1) ** 2
    if out is None:
        out = empty_nhwc(b, h, w, nk, coords)
    assert out.shape == (b, h, w, nk)
    taps = torch.empty((b * h * w, nl, 2, 2 * radius + 1), dtype=torch.int32, device=coords.device) if want_taps else None
    arr = (C.c_void_p * 4)(*[lv.data_ptr() for lv in levels] + [0] * (4 - nl))
    h0, w0 = levels[0].shape[-2:]
    _timed_call("lookup", "ff_corr_lookup_fwd", arr, nl, radius, _p(coords), b * h * w, h0, w0, _p(out), _ld(out), _p(taps), _stream())
    return (out, taps) if want_taps else out


# ----------------------------------------------------------------------------
# Zeroed fp64 statistics buffers come out of one arena per forward pass (one fill instead of one per norm layer).
# The arena is only handed out between begin_forward() and the next begin_forward(); every slice is used once.
_stats_arena = None
_stats_used = 0


def begin_forward(device):
    """Called by the model at the top of a forward pass: a fresh zeroed arena for the norm statistics."""
    global _stats_arena, _stats_used, _range_word
    _stats_arena = torch.zeros(1 << 18, dtype=torch.float64, device=device)     # 2 MB: ~60 norm layers x B x C x 2
    _stats_used = 0
    _range_word = torch.zeros(1, dtype=torch.int32, device=device) if CHECK_RANGE else None


# The split conv formats read an activation x as f16(4 x) + residual: |x| must stay below 16376 (csrc/ff_common.h), and a
# value beyond it becomes inf without any other sign than a NaN flow.  Weights are checked when they are loaded
# (model.load_state_dict); activations depend on the input, so their check is a debug mode: FF_CHECK_RANGE=1 (or
# ops.CHECK_RANGE = True) measures max|x| of every tensor a forward convolution reads (one extra read-only pass each, the
# kernel the backward uses for its gradient scales) and the model raises at the end of the forward pass that overflowed.
CHECK_RANGE = os.environ.get("FF_CHECK_RANGE", "0") == "1"
# InstanceNorm statistics from the producing convolution's epilogue (FFConvParams.stats_part) instead of a pass over its output
CONV_STATS = True
# ... and in recorded (training) passes: off - at the 46 x 62 planes of the training crop most tiles are ragged (the slow
# per-pixel branch of the epilogue) and the statistics pass it replaces is short: 70.3 vs 69.6 ms per step (A/B, round 3)
CONV_STATS_TRAIN = False
X_LIMIT = 16376.0
_range_word = None


def _range_probe(x: Tensor):
    b, h, w, c = x.shape
    if act_bwd_is_alias(x, ACT_NONE, 1.0, c):      # measures only, no copy
        _hip.call("ff_act_bwd", _p(x), _ld(x), None, 0, _p(x), c, b * h * w, c, c, ACT_NONE, 1.0, _p(_range_word), _stream())
    else:                                            # a channel slice / padded tensor: through a dense copy
        act_bwd(x, None, ACT_NONE, 1.0, c, want_amax=True, amax=_range_word)


def check_range(what: str = "forward pass"):
    """Debug mode (CHECK_RANGE): raise if an input of a split-format convolution of this pass left fp16's range."""
    if _range_word is None:
        return
    m = float(_range_word.view(torch.float32).item())       # the word holds the bits of max|x| (non-negative floats order as ints)
    if not (m < X_LIMIT):
        raise _hip.FocusFlowHipError(
            f"{what}: a convolution input reached |x| = {m:.6g}; the fp16-split conv formats need |x| < {X_LIMIT:g} "
            "(ff_common.h).  Run this checkpoint / input with FF_CONV_PRECISION=fp32.")


# ---- the always-on guard ---------------------------------------------------------------------------------------------------
# Two tensors per forward decide whether a checkpoint / input stays inside the split formats' range: the context encoder's
# output (no norm behind its last convolution: |x| ~ 700 on the synthetic test weights; slot 0) and the feature maps the
# correlation volume is built from (slot 1).  Their max|x| is measured in every forward (two read-only passes,
# ff_range_probe: ~15 us).  What happens with the two numbers depends on what is known about the model (`owner` = the RAFT
# module, which keeps the running maximum of what its forwards have shown):
#   * CAREFUL forwards - the first one after the weights changed, and every one while the running maximum is within a
#     factor 4 of the limit - read the words synchronously behind the encoders (one host sync, ~1 ms of lost run-ahead) and
#     act BEFORE the values meet a split convolution: a context output beyond the limit switches the module to its exact-fp32
#     route for the convolutions that read it (SepConvGRU.prepare: `_exact_ctx`, sticky, logged) - the flow of THAT forward is
#     right; feature maps beyond the limit have no local repair (the correlation values they produce overflow the next
#     layer as well) and raise.
#   * all other forwards copy the words to pinned host memory without a synchronisation and look at them when the NEXT
#     forward starts (or on demand: FF_RAFT_FUSION.check_range(), one host sync): a value that jumped past the limit from
#     below a quarter of it in one step raises FocusFlowHipError then - the flow of that pass was not valid - and arms the
#     exact route for what follows.
# A forward is judged by the route IT took (guard_verdict), not by what the owner's `_exact_ctx` says when the look happens:
# every queued pair of words carries that route (guard_end / guard_queue: exact_ctx, recorded).  A recorded pass has no exact
# route, so a context output beyond the limit refuses it whether the flag is armed or not; a hipGraph captured before the
# flag was armed holds the split route, so every replay of it on such inputs is refused (graph.CapturedStep remembers the
# flag as it stood at capture; capturing again after the refusal gives a graph on the exact route).
# The state lives in the per-thread policy object (two models driven from two threads do not see each other's words); hipGraph
# captures probe into static words of their own (guard_capture; graph.CapturedStep makes them) and are checked after each replay.
# Not covered: the encoders' INTERMEDIATE tensors and training tensors (debug mode FF_CHECK_RANGE=1).  FF_RANGE_GUARD=0: off.
RANGE_GUARD = os.environ.get("FF_RANGE_GUARD", "1") != "0"
GUARD_MARGIN = 4.0


def _guard_state():
    st = policy.__dict__.get("_guard")
    if st is None:
        st = policy.__dict__["_guard"] = {"words": None, "pending": [], "capture_words": None}
    return st


@contextlib.contextmanager
def guard_capture(words: Optional[Tensor]):
    """Inside the block this thread's captured forwards probe into `words` (a static int32 pair, or None: no probes); on exit,
    also by an exception, the value from before the block is back, so blocks nest."""
    st = _guard_state()
    outer, st["capture_words"] = st["capture_words"], words
    try:
        yield words
    finally:
        st["capture_words"] = outer


def guard_begin(device):
    st = _guard_state()
    st["words"] = None
    if torch.cuda.is_current_stream_capturing():      # (no event queries, host copies or fresh words inside a hipGraph capture)
        if RANGE_GUARD and st["capture_words"] is not None:
            st["words"] = st["capture_words"]
            st["words"].zero_()                         # (a captured fill: every replay starts from zero)
        return
    guard_check()
    if RANGE_GUARD:
        st["words"] = torch.zeros(2, dtype=torch.int32, device=device)


def guard_probe(x: Tensor, slot: int):
    """max|x| of an NHWC tensor into slot 0 (context encoder output) / 1 (feature maps) of the running forward's guard words."""
    w = _guard_state()["words"]
    if w is None:
        return
    b, h, ww, c = x.shape
    _hip.call("ff_range_probe", _p(x), _ld(x), b * h * ww, c, _p(w[slot:slot + 1]), _stream())


def guard_careful(owner) -> bool:
    """Should this forward read its guard words synchronously (see above)?"""
    st = _guard_state()
    if st["words"] is None or torch.cuda.is_current_stream_capturing():
        return False
    return (not getattr(owner, "_guard_hist", False)) or getattr(owner, "_guard_level", 0.0) * GUARD_MARGIN >= X_LIMIT


def guard_read_now():
    """(max|context output|, max|feature maps|) of the running forward so far: one host synchronisation."""
    w = _guard_state()["words"]
    a, b = w.view(torch.float32).tolist()
    return a, b


def guard_note(owner, m_ctx: float, m_fmap: float):
    """Fold one forward's maxima into the owner's running level."""
    m = max(m_ctx, m_fmap) if m_ctx == m_ctx and m_fmap == m_fmap else float("inf")
    owner._guard_level = max(getattr(owner, "_guard_level", 0.0), m)
    owner._guard_hist = True


GUARD_ADVICE_FP32 = "Run this checkpoint / input with FF_CONV_PRECISION=fp32."
GUARD_ADVICE_RECORDED = ("The context encoder's output left the range in a RECORDED pass; the exact-fp32 repair covers inference only.  "
                         "Train this checkpoint with FF_CONV_PRECISION=fp32.")
GUARD_ADVICE_EXACT = "The context features' convolutions run on the exact-fp32 route from now on."


def guard_verdict(m_ctx: float, m_fmap: float, exact_route: bool, recorded: bool = False):
    """The guard's decision on one forward, from its two maxima and the route it TOOK (or, in a careful forward, is about to
    take): exact_route - the context features' convolutions on the exact-fp32 rows; recorded - an autograd pass, which has no
    exact route whatever exact_route says.  -> (refuse, arm, advice): refuse - the flow of that forward is not valid; arm - the
    exact route repairs it (set the owner's `_exact_ctx`; a careful forward, which has not met a split convolution yet, takes
    it at once instead of refusing); advice - the tail of the error message.  Pure: no owner, no state."""
    if not (m_fmap < X_LIMIT) or not (m_ctx < float("inf")):
        return True, False, GUARD_ADVICE_FP32
    if m_ctx < X_LIMIT:
        return False, False, ""
    if recorded:
        return True, False, GUARD_ADVICE_RECORDED
    if exact_route:
        return False, False, ""
    return True, True, GUARD_ADVICE_EXACT


def guard_end(what: str, owner=None, handled: bool = False, exact_ctx: bool = False, recorded: bool = False):
    """End of a forward: queue its words for the asynchronous look (handled: a careful forward has read them already).
    exact_ctx / recorded: the route this forward took (guard_verdict)."""
    st = _guard_state()
    w, st["words"] = st["words"], None
    if w is None or handled or torch.cuda.is_current_stream_capturing():
        return
    guard_queue(w, what, owner, exact_ctx=exact_ctx, recorded=recorded)


def guard_queue(words: Tensor, what: str, owner=None, exact_ctx: bool = False, recorded: bool = False):
    """Copy a finished forward's pair of words to the host for guard_check, with the route that forward took: it is judged by
    that, not by what the owner's `_exact_ctx` says when the look happens."""
    host = torch.empty(2, dtype=torch.int32, pin_memory=True)
    host.copy_(words, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _guard_state()["pending"].append((host, ev, what, owner, bool(exact_ctx), bool(recorded)))


def guard_check(sync: bool = False):
    """Look at the guard words of finished forwards (all of them if sync, else those whose copy has arrived)."""
    pending = _guard_state()["pending"]
    while pending:
        host, ev, what, owner, exact_ctx, recorded = pending[0]
        if not ev.query():
            if not sync:
                return
            ev.synchronize()
        pending.pop(0)
        m_ctx, m_fmap = host.view(torch.float32).tolist()
        if owner is not None:
            guard_note(owner, m_ctx, m_fmap)
        refuse, arm, advice = guard_verdict(m_ctx, m_fmap, exact_ctx, recorded)
        if refuse:
            pending.clear()
            if owner is not None and arm:
                owner._exact_ctx = True            # the next forward of this model is right
            raise _hip.FocusFlowHipError(
                f"{what}: an encoder output reached |x| = {max(m_ctx, m_fmap):.6g}; the fp16-split conv formats need |x| < {X_LIMIT:g} "
                "(csrc/ff_common.h) - the flow of that pass is not valid.  " + advice)


def _zero_stats(s, c, device):
    global _stats_used
    n = s * c * 2
    if _stats_arena is None or _stats_arena.device != device or _stats_used + n > _stats_arena.numel():
        return torch.zeros((s, c, 2), dtype=torch.float64, device=device)
    out = _stats_arena[_stats_used:_stats_used + n].view(s, c, 2)
    _stats_used += n
    return out


BATCH_STATS_PER_IMAGE = os.environ.get("FF_BATCH_STATS_PER_IMAGE", "1") != "0"      # A/B switch


def norm_stats(x: Tensor, per_sample: bool) -> Tensor:
    b, h, w, c = x.shape
    if not per_sample and b > 1 and BATCH_STATS_PER_IMAGE:
        # batch statistics: every block of the pass ends in one fp64 atomic pair per channel, and with ONE row of sums for the whole
        # batch those chains are B times longer than an InstanceNorm's (8 x 184 x 248 x 64: 75 us, of which the bytes are worth 20 -
        # tools/norm_lab.py).  Per-image rows + a sum over them costs one small launch more and keeps the chains short.
        part = _zero_stats(b, c, x.device)
        _hip.call("ff_norm_stats", _p(x), _ld(x), b, h * w, c, 1, _p(part), _stream())
        return part.sum(0, keepdim=True)
    stats = _zero_stats(b if per_sample else 1, c, x.device)
    _hip.call("ff_norm_stats", _p(x), _ld(x), b, h * w, c, int(per_sample), _p(stats), _stream())
    return stats


def norm_coeffs(stats: Tensor, count: int, eps: float = 1e-5, gamma=None, beta=None):
    """The (scale, shift) tables norm_apply would use, fp32 [S][C] each, for conv2d(in_scale=..., in_shift=...)."""
    s_, c, _ = stats.shape
    out = torch.empty((2, s_, c), dtype=torch.float32, device=stats.device)
    _hip.call("ff_norm_coeffs", _p(stats), s_, c, count, eps, _p(gamma), _p(beta), _p(out[0]), _p(out[1]), _stream())
    return out[0], out[1]


def norm_apply(x: Tensor, stats: Tensor, per_sample: bool, eps: float = 1e-5, gamma=None, beta=None,
               act: int = ACT_NONE, res: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    b, h, w, c = x.shape
    if out is None:
        out = empty_nhwc(b, h, w, c, x)
    _hip.call("ff_norm_apply", _p(x), _ld(x), _p(out), _ld(out), b, h * w, c, _p(stats), int(per_sample), eps,
              _p(gamma), _p(beta), act, _p(res), _ld(res) if res is not None else 0, _stream())
    return out


def bn_fold(bn: torch.nn.BatchNorm2d):
    """Eval-mode BatchNorm as per-channel (scale, shift) for the conv epilogue; cached until a parameter or
    running statistic changes (version counters / storage)."""
    key = tuple((t._version, t.data_ptr()) for t in (bn.running_mean, bn.running_var, bn.weight, bn.bias))
    cached = getattr(bn, "_ff_fold", None)
    if cached is not None and cached[0] == key:
        return cached[1], cached[2]
    c = bn.num_features
    sc = torch.empty(c, dtype=torch.float32, device=bn.weight.device)
    sh = torch.empty_like(sc)
    _require_gpu(bn.weight)
    _hip.call("ff_bn_fold", _p(bn.running_mean), _p(bn.running_var), _p(bn.weight), _p(bn.bias), bn.eps, _p(sc),
              _p(sh), c, _stream())
    bn._ff_fold = (key, sc, sh)
    return sc, sh


def bn_update_running(bn: torch.nn.BatchNorm2d, stats: Tensor, count: int):
    _hip.call("ff_bn_update_running", _p(stats), count, bn.momentum, _p(bn.running_mean), _p(bn.running_var),
              bn.num_features, _stream())
    for t in (bn.running_mean, bn.running_var):     # written through raw pointers: tell PyTorch (bn_fold's cache key)
        torch.autograd.graph.increment_version(t)


# ----------------------------------------------------------------------------
def prep_input(src_nchw: Optional[Tensor], b, h, w, like: Tensor, fill: float = 0.0, out: Optional[Tensor] = None) -> Tensor:
    dst = empty_nhwc(b, h, w, 4, like) if out is None else out
    assert dst.shape == (b, h, w, 4) and dst.is_contiguous()
    if src_nchw is not None:
        _require_gpu(src_nchw)
        src_nchw = src_nchw.contiguous()
        assert src_nchw.shape[0] == b and src_nchw.shape[2:] == (h, w)
    _hip.call("ff_prep_input", _p(src_nchw), src_nchw.shape[1] if src_nchw is not None else 0, fill, _p(dst), b, h, w,
              _stream())
    return dst


def cat_batch(a: Tensor, b: Tensor) -> Tensor:
    """torch.cat([a, b], 0) - without the copy when b lies right behind a in one buffer (the model prepares both frames of a
    pair into the two halves of one tensor, so that the feature encoder sees them as ONE batch of 2B, raft.py:187-189)."""
    if (a.is_contiguous() and b.is_contiguous() and a.shape[1:] == b.shape[1:] and a.dtype == b.dtype
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and b.storage_offset() == a.storage_offset() + a.numel()):
        return torch.as_strided(a, (a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), a.stride(), a.storage_offset())
    return torch.cat([a, b], 0)


def mask_prepare(mode: int, mask_nchw: Tensor, image: Tensor, table: Tensor, raw: bool = False, image_nhwc4: bool = False) -> Tensor:
    """init_mask modes neighborG(0)/neighborE(1)/context(2) -> NHWC4; scaled to [-1,1] (FF-RAFT) or raw [0,255] (FF-PWC);
    the context image is NCHW (B,3,H,W) or, with image_nhwc4, an NHWC4 tensor."""
    _require_gpu(mask_nchw)
    b, _, h, w = mask_nchw.shape
    dst = empty_nhwc(b, h, w, 4, mask_nchw)
    tmp = torch.empty((b, h, w), dtype=torch.float32, device=mask_nchw.device)
    gmax = torch.empty(1, dtype=torch.int32, device=mask_nchw.device)
    _hip.call("ff_mask_prepare", mode | (4 if raw else 0) | (8 if image_nhwc4 else 0), _p(mask_nchw.contiguous()), _p(image.contiguous()),
              _p(table), table.shape[0], _p(tmp), _p(gmax), _p(dst), b, h, w, _stream())
    return dst


# ----------------------------------------------------------------------------
# SA / CA fusion units (parallel_fusion.py:14-73)
# ----------------------------------------------------------------------------
SPATIAL_SLABS = 64   # FF_SPATIAL_SLABS


def chan_stats(x: Tensor):
    """(B,H,W,C) -> ((B,H,W,4) = [mean_c, max_c, 0, 0], argmax (B,H,W) int32)."""
    _require_gpu(x)
    b, h, w, c = x.shape
    st = empty_nhwc(b, h, w, 4, x)
    am = torch.empty((b, h, w), dtype=torch.int32, device=x.device)
    _hip.call("ff_chan_stats_fwd", _p(x), _ld(x), c, b * h * w, _p(st), 4, _p(am), _stream())
    return st, am


def chan_stats_bwd(g: Tensor, argmax: Tensor, c: int) -> Tensor:
    b, h, w, _ = g.shape
    gx = empty_nhwc(b, h, w, c, g)
    _hip.call("ff_chan_stats_bwd", _p(g), _ld(g), _p(argmax), c, b * h * w, _p(gx), _ld(gx), _stream())
    return gx


def _spatial_scratch(b, c, like):
    return torch.empty(SPATIAL_SLABS * b * c * 3, dtype=torch.float32, device=like.device)


def spatial_stats(x: Tensor):
    """(B,H,W,C) -> ((2B,1,1,C): rows [0,B) = mean over pixels, rows [B,2B) = max; argmax (B,C) int32)."""
    _require_gpu(x)
    b, h, w, c = x.shape
    out = torch.empty((2 * b, 1, 1, c), dtype=torch.float32, device=x.device)
    am = torch.empty((b, c), dtype=torch.int32, device=x.device)
    _hip.call("ff_spatial_stats_fwd", _p(x), _ld(x), c, b, h * w, _p(out), _p(out[b:]), _p(am), _p(_spatial_scratch(b, c, x)),
              _stream())
    return out, am


def spatial_stats_bwd(g: Tensor, argmax: Tensor, h: int, w: int) -> Tensor:
    b2, _, _, c = g.shape
    b = b2 // 2
    g = g.contiguous()
    gx = empty_nhwc(b, h, w, c, g)
    _hip.call("ff_spatial_stats_bwd", _p(g), _p(g[b:]), _p(argmax), c, b, h * w, _p(gx), _ld(gx), _stream())
    return gx


def scale_add(v: Tensor, s: Tensor, q: Optional[Tensor], mode: int) -> Tensor:
    """out = s * v + q.  mode 0: s (B,H,W,1) per pixel; mode 1: s (2B,1,1,C), scale = s[:B] + s[B:]."""
    _require_gpu(v)
    b, h, w, c = v.shape
    out = empty_nhwc(b, h, w, c, v)
    if mode == 0:
        assert s.shape[:3] == (b, h, w)
        _hip.call("ff_scale_add_fwd", _p(v), _ld(v), _p(s), _ld(s), None, _p(q), _ld(q) if q is not None else 0, _p(out),
                  _ld(out), c, b, h * w, 0, _stream())
    else:
        assert s.shape == (2 * b, 1, 1, c) and s.is_contiguous()
        _hip.call("ff_scale_add_fwd", _p(v), _ld(v), _p(s), 0, _p(s[b:]), _p(q), _ld(q) if q is not None else 0, _p(out),
                  _ld(out), c, b, h * w, 1, _stream())
    return out


def scale_add_bwd(gout: Tensor, v: Tensor, s: Tensor, mode: int):
    """-> (gv, gs) with gs shaped like s."""
    b, h, w, c = v.shape
    gv = empty_nhwc(b, h, w, c, v)
    if mode == 0:
        gs = torch.empty((b, h, w, 1), dtype=torch.float32, device=v.device)
        _hip.call("ff_scale_add_bwd", _p(gout), _ld(gout), _p(v), _ld(v), _p(s), _ld(s), None, _p(gv), _ld(gv), _p(gs), None,
                  c, b, h * w, 0, _stream())
    else:
        gs = torch.empty((2 * b, 1, 1, c), dtype=torch.float32, device=v.device)
        _hip.call("ff_scale_add_bwd", _p(gout), _ld(gout), _p(v), _ld(v), _p(s), 0, _p(s[b:]), _p(gv), _ld(gv), _p(gs),
                  _p(_spatial_scratch(b, c, v)), c, b, h * w, 1, _stream())
    return gv, gs


def act_copy(src: Tensor, dst: Tensor, act: int):
    b, h, w, c = src.shape
    assert dst.shape == src.shape
    _hip.call("ff_act_copy", _p(src), _ld(src), _p(dst), _ld(dst), b * h * w, c, act, _stream())


def coords_init(b, h, w, like: Tensor, flow_init: Optional[Tensor] = None) -> Tensor:
    coords = empty_nhwc(b, h, w, 2, like)
    if flow_init is not None:
        _require_gpu(flow_init)
        flow_init = flow_init.contiguous()
        assert flow_init.shape == (b, 2, h, w)
    _hip.call("ff_coords_init", _p(coords), _p(flow_init), b, h, w, _stream())
    return coords


def forward_interpolate(flow: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """utils.forward_interpolate (utils.py:26-54) on the device: the 1/8-resolution flow of one pair -> the flow_init of the
    next.  flow: (2,H,W) or (B,2,H,W), any strides; out: a contiguous tensor of the same shape (default: a new one; may be
    `flow` itself).  Bit-equal to an fp64 brute-force nearest neighbour with ties to the lowest source index; a sample of
    which no vector lands gives zeros where scipy gives NaN (csrc/warm_start.hip)."""
    _require_gpu(flow)
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise _hip.FocusFlowHipError(f"forward_interpolate: (2,H,W) or (B,2,H,W) expected, got {tuple(flow.shape)}")
    src = flow.contiguous()
    out = torch.empty_like(src) if out is None else _arg("forward_interpolate", "out", out, (torch.float32,), tuple(flow.shape), contiguous=True)
    b = src.shape[0] if src.dim() == 4 else 1
    h, w = src.shape[-2:]
    nbytes = _hip.load().ff_forward_interpolate_ws(b, h, w)
    if nbytes <= 0:
        raise _hip.FocusFlowHipError(f"forward_interpolate: shape {tuple(flow.shape)} is not supported")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    _hip.call("ff_forward_interpolate", _p(src), _p(out), _p(ws), b, h, w, _stream())
    return out


def good_features_ws(b: int, h: int, w: int) -> int:
    """Bytes of workspace ff_good_features needs for (B, H, W); 0: the shape is not supported."""
    return _hip.load().ff_good_features_ws(b, h, w)


def good_features(image: Tensor, max_corners: int = 500, quality_level: float = 0.01, min_distance: int = 10,
                  out: Optional[Tensor] = None, return_points: bool = False, ws: Optional[Tensor] = None):
    """Shi-Tomasi key points as a mask (csrc/keypoints.hip): what scripts/maskGenerate.py makes offline with
    cv.goodFeaturesToTrack(img, 500, 0.01, 10).  image: (B,3,H,W) R,G,B or (B,1,H,W) fp32 in [0,255], any strides with a
    dense innermost dimension; out: a contiguous (B,1,H,W) fp32 tensor (default: a new one).  -> mask (255 at key points,
    0 elsewhere), or (mask, points (B,max_corners,2) int32 [x, y] in acceptance order and -1 beyond the count, count (B)
    int32).  ws: a uint8 device tensor of good_features_ws(B, H, W) bytes to work in (default: a new one per call).
    Exact: equal to the integer / fp64 definition bit for bit.  Enqueues only, so it can be captured."""
    _require_gpu(image)
    if image.dim() != 4:
        raise _hip.FocusFlowHipError(f"good_features: (B,1,H,W) or (B,3,H,W) expected, got {tuple(image.shape)}")
    b, c, h, w = image.shape
    if w > 1 and image.stride(3) != 1:
        image = image.contiguous()
    out = torch.empty((b, 1, h, w), dtype=torch.float32, device=image.device) if out is None else \
        _arg("good_features", "out", out, (torch.float32,), (b, 1, h, w), contiguous=True)
    points = count = None
    if return_points and max_corners >= 1:
        points = torch.empty((b, max_corners, 2), dtype=torch.int32, device=image.device)
        count = torch.empty((b,), dtype=torch.int32, device=image.device)
    ws = _workspace("good_features", ws, good_features_ws(b, h, w), image.device)
    _hip.call("ff_good_features", _p(image), c, image.stride(0), image.stride(1), image.stride(2), b, h, w, int(max_corners),
              float(quality_level), int(min_distance), _p(ws), _p(out), _p(points), _p(count), _stream())
    return (out, points, count) if return_points else out


def pad_offsets(h: int, w: int, pad_mode: str = "sintel"):
    """(left, top, Hp, Wp) of utils.InputPadder((h, w), pad_mode): replicate padding to multiples of 8, centred for
    'sintel', at the bottom (and centred horizontally) for anything else (KITTI)."""
    pad_h, pad_w = (-h) % 8, (-w) % 8
    return pad_w // 2, (pad_h // 2 if pad_mode == "sintel" else 0), h + pad_h, w + pad_w


# ---- the arguments of the session wrappers -----------------------------------------------------------------------------------
def _arg(name: str, what: str, t, dtypes, shape=None, device=None, contiguous: bool = False) -> Tensor:
    """The one check of a tensor argument: `what` of the entry `name` must be a tensor on a HIP device with one of `dtypes` and,
    where given, of `shape` (an int per dimension, or a letter for a size that is free: ("B", "N", 2)), on `device`, contiguous.
    -> t, or a FocusFlowHipError that names the entry, the argument, all that was asked and what came."""
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise _hip.FocusFlowHipError(f"{name}: {what} must be a tensor on a HIP device (got {'a CPU tensor' if isinstance(t, Tensor) else type(t).__name__}); "
                                     "there is no CPU fallback")
    fits = shape is None or (t.dim() == len(shape) and all(isinstance(s, str) or s == d for s, d in zip(shape, t.shape)))
    if t.dtype not in dtypes or not fits or (device is not None and t.device != device) or (contiguous and not t.is_contiguous()):
        asked = ("contiguous " if contiguous else "") + " or ".join(str(d) for d in dtypes)
        asked += "" if shape is None else " (" + ",".join(str(s) for s in shape) + ("," if len(shape) == 1 else "") + ")"
        raise _hip.FocusFlowHipError(f"{name}: {what} must be {asked}{'' if device is None else f' on {device}'}, "
                                     f"got {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    return t


def _outs(name: str, out, specs, device):
    """out: None (new tensors) or one contiguous tensor per (what, shape, dtype) of `specs`, on `device`.  -> the tuple"""
    if out is None:
        return tuple(torch.empty(shape, dtype=dtype, device=device) for _, shape, dtype in specs)
    if not isinstance(out, (tuple, list)) or len(out) != len(specs):
        raise _hip.FocusFlowHipError(f"{name}: out must be the tuple ({', '.join(w for w, _, _ in specs)})")
    return tuple(_arg(name, f"out ({what})", t, (dtype,), tuple(shape), device, contiguous=True) for t, (what, shape, dtype) in zip(out, specs))


def _out(name: str, out: Optional[Tensor], shape, device, dtype=torch.float32) -> Tensor:
    """out: None (a new tensor) or the contiguous `dtype` tensor of `shape` on `device` to write into."""
    return torch.empty(shape, dtype=dtype, device=device) if out is None else _arg(name, "out", out, (dtype,), tuple(shape), device, contiguous=True)


def _workspace(name: str, ws: Optional[Tensor], nbytes: int, device) -> Tensor:
    """ws: None (a new one) or a contiguous uint8 tensor of at least `nbytes` bytes on `device` to work in."""
    if ws is None:
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)      # (an unsupported shape is refused by the call itself, with its reason)
    if _arg(name, "ws", ws, (torch.uint8,), None, device, contiguous=True).numel() < nbytes:
        raise _hip.FocusFlowHipError(f"{name}: ws must hold at least {nbytes} bytes, got {ws.numel()}")
    return ws


def _frame_in_field(name: str, what: str, t, left, top, h=None, w=None, shape=("B", 2, "Hp", "Wp"), device=None):
    """A padded (B,2,Hp,Wp) fp32 flow field of any strides whose h x w frame starts at (left, top) (default: everything right of
    and below it), as every C entry takes it: -> (pointer, the four element strides, B, left, top, h, w, Hp, Wp).  Checks the
    field's shape; whether the frame lies inside the field is the library's to refuse."""
    b, _, hp, wp = _arg(name, what, t, (torch.float32,), shape, device).shape
    left, top = int(left), int(top)
    return (_p(t), *t.stride(), b, left, top, hp - top if h is None else int(h), wp - left if w is None else int(w), hp, wp)


def frame_ingest(frame: Tensor, layout: str = "hwc", order: str = "rgb", pad_mode: str = "sintel", out: Optional[Tensor] = None) -> Tensor:
    """A decoder's uint8 frame -> the fp32 (B,3,Hp,Wp) R,G,B tensor the models take (csrc/frame_io.hip): what
    x.permute(0, 3, 1, 2).float() and utils.InputPadder(x.shape, pad_mode).pad do, bit for bit, in one launch.
    frame: uint8 (B,H,W,3) / (H,W,3) for layout 'hwc', (B,3,H,W) / (3,H,W) for 'chw', any strides (a crop, the [..., :3]
    view of an RGBA frame); order 'rgb' or 'bgr'; out: a contiguous fp32 (B,3,Hp,Wp) tensor (default: a new one).
    Enqueues only, so it can be captured."""
    _arg("frame_ingest", "frame", frame, (torch.uint8,))
    if layout not in ("hwc", "chw"):
        raise _hip.FocusFlowHipError(f"frame_ingest: layout = {layout!r} ('hwc' or 'chw')")
    if order not in ("rgb", "bgr"):
        raise _hip.FocusFlowHipError(f"frame_ingest: order = {order!r} ('rgb' or 'bgr')")
    if frame.dim() == 3:
        frame = frame.unsqueeze(0)
    if frame.dim() != 4:
        raise _hip.FocusFlowHipError(f"frame_ingest: frame must be (B,H,W,3) / (H,W,3) [hwc] or (B,3,H,W) / (3,H,W) [chw], got {tuple(frame.shape)}")
    if layout == "hwc":
        b, h, w, c = frame.shape
        ld_b, ld_row, ld_col, ld_c = frame.stride()
    else:
        b, c, h, w = frame.shape
        ld_b, ld_c, ld_row, ld_col = frame.stride()
    if c != 3:
        raise _hip.FocusFlowHipError(f"frame_ingest: frame has {c} channels in layout {layout!r}, shape {tuple(frame.shape)}: 3 expected "
                                     "(take frame[..., :3] of an RGBA frame)")
    left, top, hp, wp = pad_offsets(h, w, pad_mode)
    out = _out("frame_ingest", out, (b, 3, hp, wp), frame.device)
    _hip.call("ff_frame_ingest", _p(frame), ld_b, ld_row, ld_col, ld_c, int(order == "bgr"), b, h, w, left, top, hp, wp, _p(out), _stream())
    return out


def pad_replicate(mask: Tensor, pad_mode: str = "sintel", out: Optional[Tensor] = None) -> Tensor:
    """utils.InputPadder(mask.shape, pad_mode).pad for a one-channel mask, into fp32 (csrc/frame_io.hip): mask (B,1,H,W) or
    (B,H,W), uint8 or fp32, any strides; out: a contiguous fp32 (B,1,Hp,Wp) tensor (default: a new one).  Bit-identical to
    F.pad(mask.float(), mode='replicate').  Enqueues only, so it can be captured."""
    _arg("pad_replicate", "mask", mask, (torch.uint8, torch.float32))
    if mask.dim() == 4 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if mask.dim() != 3:
        raise _hip.FocusFlowHipError(f"pad_replicate: mask must be (B,1,H,W) or (B,H,W), got {tuple(mask.shape)}")
    b, h, w = mask.shape
    left, top, hp, wp = pad_offsets(h, w, pad_mode)
    out = _out("pad_replicate", out, (b, 1, hp, wp), mask.device)
    _hip.call("ff_pad_replicate", _p(mask), int(mask.dtype == torch.uint8), mask.stride(0), mask.stride(1), mask.stride(2), b, h, w, left, top, hp, wp,
              _p(out), _stream())
    return out


def keypoint_matches(points: Tensor, count: Tensor, flow_up: Tensor, left: int, top: int, h: int, w: int,
                     out: Optional[Tensor] = None, valid: Optional[Tensor] = None):
    """The flow at key points as matches (csrc/frame_io.hip).  points (B,N,2) int32 [x, y] and count (B) int32 as
    good_features(return_points=True) gives them, in coordinates of the unpadded h x w frame; flow_up (B,2,Hp,Wp) fp32, any
    strides, the padded field whose frame starts at (left, top).  -> (matches (B,N,4) fp32 [x, y, x + u, y + v], valid (B,N)
    uint8: the target lies inside the frame); rows from count[b] on hold -1 and 0.  out / valid: contiguous tensors to
    write into (default: new ones).  Enqueues only, so it can be captured."""
    name = "keypoint_matches"
    b, n, _ = _arg(name, "points", points, (torch.int32,), ("B", "N", 2), contiguous=True).shape
    dev = points.device
    _arg(name, "count", count, (torch.int32,), (b,), contiguous=True)
    field = _frame_in_field(name, "flow_up", flow_up, left, top, h, w, shape=(b, 2, "Hp", "Wp"))
    out = _out(name, out, (b, n, 4), dev)
    valid = torch.empty((b, n), dtype=torch.uint8, device=dev) if valid is None else _arg(name, "valid", valid, (torch.uint8,), (b, n), dev, contiguous=True)
    _hip.call("ff_keypoint_matches", _p(points), _p(count), n, *field, _p(out), _p(valid), _stream())
    return out, valid


def _track_table(name: str, pos: Tensor, ids: Tensor, age: Optional[Tensor] = None):
    """The shapes of a track table's state (tracks.TrackTable): -> (B, N)."""
    b, n, _ = _arg(name, "pos", pos, (torch.float32,), ("B", "N", 2), contiguous=True).shape
    _arg(name, "ids", ids, (torch.int64,), (b, n), pos.device, contiguous=True)
    if age is not None:
        _arg(name, "age", age, (torch.int32,), (b, n), pos.device, contiguous=True)
    return b, n


def _match_rows(name: str, matches: Tensor, valid: Tensor, table):
    """What fb_matches, epipolar_ransac and homography_ransac ask of a matches / valid pair and of table: None or the (pos, ids,
    age) of a track table whose slots are the rows.  -> (B, N, device, pos, ids, age)"""
    b, n, _ = _arg(name, "matches", matches, (torch.float32,), ("B", "N", 4), contiguous=True).shape
    dev = matches.device
    _arg(name, "valid", valid, (torch.uint8,), (b, n), dev, contiguous=True)
    pos = ids = age = None
    if table is not None:
        if not isinstance(table, (tuple, list)) or len(table) != 3 or any(t is None for t in table):
            raise _hip.FocusFlowHipError(f"{name}: table must be the tuple (pos, ids, age) of a track table, all three, or None")
        pos, ids, age = table
        if _track_table(name, pos, ids, age) != (b, n) or pos.device != dev:
            raise _hip.FocusFlowHipError(f"{name}: table must have the rows of matches, {(b, n)} on {dev}, got pos {tuple(pos.shape)} on {pos.device}")
    return b, n, dev, pos, ids, age


def tracks_replenish(pos: Tensor, ids: Tensor, age: Tensor, next_id: Tensor, points: Tensor, count: Tensor, h: int, w: int,
                     min_distance: int, out=None):
    """Fill the free slots of a track table with the detector's points (csrc/tracks.hip; the definition is in
    include/focusflow_hip.h).  pos (B,N,2) fp32, ids (B,N) int64, age (B,N) int32, next_id (B) int64: the table, updated in
    place; points (B,M,2) int32 and count (B) int32 as good_features(return_points=True) gives them, in coordinates of the h x w
    frame.  A detection nearer than min_distance to a track that was live before the call is blocked; the others take the
    free slots in ascending order and ids from next_id on.  -> (born (B) int32, live (B) int32); out: that tuple to write
    into (default: new tensors).  Exact.  Enqueues only, so it can be captured."""
    name = "tracks_replenish"
    b, n = _track_table(name, pos, ids, age)
    _arg(name, "next_id", next_id, (torch.int64,), (b,), pos.device, contiguous=True)
    _arg(name, "points", points, (torch.int32,), (b, "M", 2), pos.device, contiguous=True)
    _arg(name, "count", count, (torch.int32,), (b,), pos.device, contiguous=True)
    born, live = _outs(name, out, (("born", (b,), torch.int32), ("live", (b,), torch.int32)), pos.device)
    _hip.call("ff_tracks_replenish", _p(pos), _p(ids), _p(age), _p(next_id), n, _p(points), _p(count), points.shape[1], b, int(h), int(w),
              int(min_distance), _p(born), _p(live), _stream())
    return born, live


def tracks_mask(pos: Tensor, ids: Tensor, h: int, w: int, out: Optional[Tensor] = None) -> Tensor:
    """The live tracks as a key-point mask (csrc/tracks.hip): (B,1,h,w) fp32, 0 everywhere and 255 at the pixel nearest to
    every live slot's position (floorf(x + 0.5f), clamped into the frame).  out: a contiguous (B,1,h,w) fp32 tensor (default: a
    new one).  Enqueues only, so it can be captured."""
    b, _ = _track_table("tracks_mask", pos, ids)
    out = _out("tracks_mask", out, (b, 1, int(h), int(w)), pos.device)
    _hip.call("ff_tracks_mask", _p(pos), _p(ids), pos.shape[1], b, int(h), int(w), _p(out), _stream())
    return out


def tracks_advance(pos: Tensor, ids: Tensor, age: Tensor, flow_up: Tensor, left: int, top: int, h: int, w: int, out=None):
    """Move every live track by the flow at its position (csrc/tracks.hip; the definition is in include/focusflow_hip.h).
    The table (pos, ids, age) is updated in place; flow_up (B,2,Hp,Wp) fp32, any strides, the padded field whose h x w frame
    starts at (left, top), sampled bilinearly in fp32 without leaving the frame.  -> (matches (B,N,4) fp32 [x, y, x', y'], valid
    (B,N) uint8, ids (B,N) int64 and age (B,N) int32 as they were before the advance); rows of dead slots hold -1, 0, -1, 0.  A
    track whose target leaves the frame (or is a NaN) dies.  out: that tuple of four to write into (default: new tensors).
    Exact.  Enqueues only, so it can be captured."""
    name = "tracks_advance"
    b, n = _track_table(name, pos, ids, age)
    field = _frame_in_field(name, "flow_up", flow_up, left, top, h, w, shape=(b, 2, "Hp", "Wp"), device=pos.device)
    matches, valid, ids_out, age_out = _outs(name, out, (("matches", (b, n, 4), torch.float32), ("valid", (b, n), torch.uint8),
                                                         ("ids", (b, n), torch.int64), ("age", (b, n), torch.int32)), pos.device)
    _hip.call("ff_tracks_advance", _p(pos), _p(ids), _p(age), n, *field, _p(matches), _p(valid), _p(ids_out), _p(age_out), _stream())
    return matches, valid, ids_out, age_out


def fb_dense(fw: Tensor, bw: Tensor, left: int, top: int, h: int, w: int, alpha: float = 0.01, beta: float = 0.5, out=None):
    """The forward-backward check of every pixel (csrc/fb_check.hip; the definition is in include/focusflow_hip.h).  fw, bw:
    (B,2,Hp,Wp) fp32, any strides (independent of each other), the padded forward and backward fields whose h x w frame starts
    at (left, top).  A pixel goes to its target by fw and comes back by bw sampled bilinearly there; it is occluded where the
    squared round-trip error exceeds alpha (|fw|^2 + |bw|^2) + beta, or the target lies outside the frame.  -> (err2 (B,1,h,w)
    fp32, +inf outside the frame; occluded (B,1,h,w) uint8, 1 or 0); out: that tuple to write into (default: new tensors).
    Exact.  Enqueues only, so it can be captured."""
    name = "fb_dense"
    fw_field = _frame_in_field(name, "fw", fw, left, top, h, w)
    b, _, _, h, w, hp, wp = fw_field[5:]
    bw_field = _frame_in_field(name, "bw", bw, left, top, h, w, shape=(b, 2, hp, wp), device=fw.device)
    err2, occluded = _outs(name, out, (("err2", (b, 1, h, w), torch.float32), ("occluded", (b, 1, h, w), torch.uint8)), fw.device)
    _hip.call("ff_fb_dense", *fw_field[:5], *bw_field, float(alpha), float(beta), _p(err2), _p(occluded), _stream())
    return err2, occluded


def fb_matches(matches: Tensor, valid: Tensor, bw: Tensor, left: int, top: int, h: int, w: int, alpha: float = 0.01, beta: float = 0.5,
               table=None, out=None):
    """The forward-backward check of the rows of a matches / valid pair (csrc/fb_check.hip; the definition is in
    include/focusflow_hip.h).  matches (B,N,4) fp32 [x, y, x', y'] and valid (B,N) uint8 as keypoint_matches or tracks_advance
    gave them; bw (B,2,Hp,Wp) fp32, any strides, the padded backward field whose h x w frame starts at (left, top).  `valid` is
    updated in place: cleared where the round trip is inconsistent.  table: None, or (pos, ids, age) of a track table whose
    slots are the rows: the slot of an inconsistent row dies, every other slot is left alone.  -> (err2 (B,N) fp32: -1 for no
    row, +inf where the target left the frame; status (B,N) uint8: 0 no row, 1 consistent, 2 the target left the frame, 3
    inconsistent); out: that tuple to write into (default: new tensors).  Exact.  Enqueues only, so it can be captured."""
    name = "fb_matches"
    b, n, dev, pos, ids, age = _match_rows(name, matches, valid, table)
    field = _frame_in_field(name, "bw", bw, left, top, h, w, shape=(b, 2, "Hp", "Wp"), device=dev)
    err2, status = _outs(name, out, (("err2", (b, n), torch.float32), ("status", (b, n), torch.uint8)), dev)
    _hip.call("ff_fb_matches", _p(matches), _p(valid), n, *field, float(alpha), float(beta), _p(pos), _p(ids), _p(age), _p(err2), _p(status), _stream())
    return err2, status


def flow_to_image(flow: Tensor, left: int = 0, top: int = 0, h: Optional[int] = None, w: Optional[int] = None, max_flow: Optional[float] = None,
                  clip_flow: Optional[float] = None, order: str = "rgb", layout: str = "hwc", occluded: Optional[Tensor] = None,
                  occluded_color=(0, 0, 0), out: Optional[Tensor] = None, return_max: bool = False):
    """A flow field as colours by the Middlebury colour wheel (csrc/flow_viz.hip; the definition is in include/focusflow_hip.h):
    the reference's flow_viz.flow_to_image on the device, uint8 out.  flow: (B,2,Hp,Wp) fp32, any strides, the padded field whose
    h x w frame starts at (left, top) (default: everything right of and below (left, top)).  Every sample is scaled by the
    maximum magnitude of ITS frame, or by max_flow (finite, > 0) where that is given: a fixed scale, beyond which vectors are
    darkened instead, so that the colours of a video do not pump.  clip_flow (>= 0): np.clip(flow, 0, clip_flow) first, as the
    reference does it.  order 'rgb' or 'bgr'; layout 'hwc': (B,h,w,3), 'chw': (B,3,h,w).  occluded: None, or a uint8 (B,1,h,w) /
    (B,h,w) plane, any strides: where it is non-zero the pixel is occluded_color, an (r, g, b) triple of 0 .. 255.  A vector with
    a non-finite component is left out of the maximum and painted black.  out: a uint8 tensor of the layout's shape, any strides
    (default: a new contiguous one), or with return_max the tuple (image, rad_max) to write into.  -> the image, or with
    return_max (image, rad_max (B) fp32: the maxima of the frames, whether or not max_flow replaced them as the scale).  Two
    launches (one with max_flow and without return_max); enqueues only, so it can be captured."""
    name = "flow_to_image"
    field = _frame_in_field(name, "flow", flow, left, top, h, w)
    b, left, top, h, w, hp, wp = field[5:]
    dev = flow.device
    if left < 0 or top < 0 or h < 1 or w < 1 or left + w > wp or top + h > hp:
        raise _hip.FocusFlowHipError(f"{name}: the {h} x {w} frame at (left, top) = ({left}, {top}) does not lie inside the {hp} x {wp} field")
    if max_flow is not None and not (float(max_flow) > 0 and math.isfinite(float(max_flow))):
        raise _hip.FocusFlowHipError(f"{name}: max_flow = {max_flow}: None (the maximum of every frame) or a finite value > 0")
    if clip_flow is not None and not float(clip_flow) >= 0:
        raise _hip.FocusFlowHipError(f"{name}: clip_flow = {clip_flow}: None or a value >= 0")
    if order not in ("rgb", "bgr"):
        raise _hip.FocusFlowHipError(f"{name}: order = {order!r} ('rgb' or 'bgr')")
    if layout not in ("hwc", "chw"):
        raise _hip.FocusFlowHipError(f"{name}: layout = {layout!r} ('hwc' or 'chw')")
    occ_ld = (0, 0, 0)
    if occluded is not None:
        if isinstance(occluded, Tensor) and occluded.dim() == 4 and occluded.shape[1] == 1:      # (B,1,h,w) is taken as (B,h,w)
            occluded = occluded[:, 0]
        occ_ld = _arg(name, "occluded", occluded, (torch.uint8,), (b, h, w), dev).stride()
    try:
        color = tuple(int(c) for c in occluded_color)
        exact = all(c == x for c, x in zip(color, occluded_color))
    except (TypeError, ValueError):
        color, exact = (), False
    if len(color) != 3 or not exact or not all(0 <= c <= 255 for c in color):
        raise _hip.FocusFlowHipError(f"{name}: occluded_color = {occluded_color!r}: an (r, g, b) triple of integers 0 .. 255")
    shape = (b, h, w, 3) if layout == "hwc" else (b, 3, h, w)
    rad_max = None
    if isinstance(out, (tuple, list)):      # (image, rad_max): a session's static buffers
        if not return_max or len(out) != 2:
            raise _hip.FocusFlowHipError(f"{name}: out must be the image, or with return_max the tuple (image, rad_max)")
        out, rad_max = out
        _arg(name, "out (rad_max)", rad_max, (torch.float32,), (b,), dev, contiguous=True)
    out = torch.empty(shape, dtype=torch.uint8, device=dev) if out is None else _arg(name, f"out (layout {layout!r})", out, (torch.uint8,), shape, dev)
    ld_b, ld_row, ld_col, ld_c = out.stride() if layout == "hwc" else (out.stride(0), out.stride(2), out.stride(3), out.stride(1))
    clip = -1.0 if clip_flow is None else float(clip_flow)
    if max_flow is None or return_max:
        if rad_max is None:
            rad_max = torch.empty((b,), dtype=torch.float32, device=dev)
        _hip.call("ff_flow_rad_max", *field, clip, _p(rad_max), _stream())
    _hip.call("ff_flow_to_image", *field, _p(rad_max if max_flow is None else None), 0.0 if max_flow is None else float(max_flow), clip,
              _p(occluded), *occ_ld, *color, int(order == "bgr"), _p(out), ld_b, ld_row, ld_col, ld_c, _stream())
    return (out, rad_max) if return_max else out


def epipolar_ws(b: int, n: int, hypotheses: int) -> int:
    """Bytes of workspace ff_epipolar_ransac needs for (B, N, K); 0: the shape is not supported."""
    return _hip.load().ff_epipolar_ws(int(b), int(n), int(hypotheses))


def _ransac(check: str, model: str, matches: Tensor, valid: Tensor, h, w, threshold, hypotheses, min_inliers, permilles, seed, epoch: Tensor, table, cull,
            out, ws: Optional[Tensor], hold: Optional[Tensor] = None):
    """The body of epipolar_ransac and homography_ransac: ff_<check>_ransac on a matches / valid pair.  model: the name of the
    (B,3,3) output; permilles: (permille,), or (permille, planar_permille) for a check with a `planar` output.  -> the outputs"""
    name = f"{check}_ransac"
    b, n, dev, pos, ids, age = _match_rows(name, matches, valid, table)
    if _arg(name, "epoch", epoch, (torch.int32,), None, dev).numel() != 1:
        raise _hip.FocusFlowHipError(f"{name}: epoch must be one int32, got {tuple(epoch.shape)}")
    if check == "homography" and matches.data_ptr() % 16:
        raise _hip.FocusFlowHipError(f"{name}: matches must be 16-byte aligned (a view that starts inside a row is not)")
    per_sample = [("inliers", torch.int32), ("candidates", torch.int32), ("ok", torch.uint8)] + [("planar", torch.uint8)] * (len(permilles) == 2)
    res = _outs(name, out, ((model, (b, 3, 3), torch.float32), *((what, (b,), dtype) for what, dtype in per_sample),
                            ("status", (b, n), torch.uint8), ("dist2", (b, n), torch.float32)), dev)
    ws = _workspace(name, ws, getattr(_hip.load(), f"ff_{check}_ws")(b, n, int(hypotheses)), dev)
    entry, tail = f"ff_{check}_ransac", ()
    if hold is not None:
        entry, tail = entry + "_hold", (_p(_arg(name, "hold", hold, (torch.uint8,), (b,), dev, contiguous=True)),)
    m3, *per_sample, status, dist2 = res      # (the C entries take dist2 and status before the per-sample outputs)
    _hip.call(entry, _p(matches), _p(valid), b, n, int(h), int(w), float(threshold), int(hypotheses), int(min_inliers), *map(int, permilles),
              int(seed) & 0xffffffff, _p(epoch), int(bool(cull)), _p(pos), _p(ids), _p(age), _p(m3), _p(dist2), _p(status), *map(_p, per_sample), _p(ws),
              ws.numel(), *tail, _stream())
    return res


def epipolar_ransac(matches: Tensor, valid: Tensor, h: int, w: int, threshold: float, hypotheses: int, min_inliers: int, permille: int, seed: int,
                    epoch: Tensor, table=None, cull: bool = True, out=None, ws: Optional[Tensor] = None, hold: Optional[Tensor] = None):
    """The epipolar check of the rows of a matches / valid pair (csrc/epipolar.hip; the definition is in include/focusflow_hip.h):
    a RANSAC over `hypotheses` 8-point fundamental matrices in coordinates normalised by the h x w frame, scored by the Sampson
    distance against `threshold` px.  matches (B,N,4) fp32 [x, y, x', y'] and valid (B,N) uint8 as keypoint_matches,
    tracks_advance or fb_matches left them; the candidates are the rows with valid = 1.  There is a verdict where at least 8
    candidates exist and the best model has at least min_inliers inliers and permille / 1000 of the candidates; then `valid` is
    cleared in place where a candidate is an outlier, and with cull and a table (pos, ids, age) whose slots are the rows those
    slots die.  epoch: one int32 on the device, read by the draws and incremented by the call.  -> (F (B,3,3) fp32 in pixel
    coordinates, x'^t F x = 0, zeros without a verdict; inliers (B) int32; candidates (B) int32; ok (B) uint8; status (B,N) uint8:
    0 no row, 1 inlier, 2 not a candidate, 3 outlier, 4 candidate but no verdict; dist2 (B,N) fp32 px^2: -1 no row, +inf without a
    verdict); out: that tuple to write into (default: new tensors).  ws: a uint8 device tensor of epipolar_ws(B, N, hypotheses)
    bytes to work in (default: a new one per call).  hold: None, or (B) uint8 on the device (ff_epipolar_ransac_hold): a sample
    whose byte is not 0 gets no verdict - ok 0, F zero, valid and the table left alone -, as homography_ransac's `planar` asks
    where F is under-determined.  Exact.  Enqueues only, so it can be captured."""
    return _ransac("epipolar", "F", matches, valid, h, w, threshold, hypotheses, min_inliers, (permille,), seed, epoch, table, cull, out, ws, hold)


def homography_ws(b: int, n: int, hypotheses: int) -> int:
    """Bytes of workspace ff_homography_ransac needs for (B, N, K); 0: the shape is not supported."""
    return _hip.load().ff_homography_ws(int(b), int(n), int(hypotheses))


def homography_ransac(matches: Tensor, valid: Tensor, h: int, w: int, threshold: float, hypotheses: int, min_inliers: int, permille: int,
                      planar_permille: int, seed: int, epoch: Tensor, table=None, cull: bool = False, out=None, ws: Optional[Tensor] = None):
    """The homography check of the rows of a matches / valid pair (csrc/homography.hip; the definition is in
    include/focusflow_hip.h): a RANSAC over `hypotheses` 4-point homographies (DLT) in coordinates normalised by the h x w frame,
    scored by the transfer error in the second image against `threshold` px.  Arguments as epipolar_ransac.  There is a verdict
    where at least 4 candidates exist and the best model has at least min_inliers inliers and permille / 1000 of the candidates;
    the pair is `planar` (one plane, or a camera that only rotates) where it also has planar_permille / 1000 of them.  With a
    verdict `valid` is cleared in place where a candidate is an outlier, and with cull and a table those slots die.
    -> (H (B,3,3) fp32 in pixel coordinates, (x', y', 1) ~ H (x, y, 1), zeros without a verdict; inliers (B) int32; candidates (B)
    int32; ok (B) uint8; planar (B) uint8; status (B,N) uint8 as epipolar_ransac; dist2 (B,N) fp32 px^2: -1 no row, +inf without a
    verdict and where the map sends the point behind the plane at infinity); out: that tuple to write into.  ws: a uint8 device
    tensor of homography_ws(B, N, hypotheses) bytes.  Exact.  Enqueues only, so it can be captured."""
    return _ransac("homography", "H", matches, valid, h, w, threshold, hypotheses, min_inliers, (permille, planar_permille), seed, epoch, table, cull, out, ws)


def homography_residual(flow: Tensor, H: Tensor, ok: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """The dense residual of a flow field against the homographies of homography_ransac (csrc/homography.hip; the definition is
    in include/focusflow_hip.h).  flow (B,2,h,w) fp32 with ANY strides - the unpadded crop of a padded flow is passed as the view
    it is -, H (B,3,3) fp32 in pixel coordinates of that frame, ok (B) uint8.  -> (B,h,w) fp32: |(x + u, y + v) - pi(H (x, y, 1))|^2
    in px^2, +inf where the map's w <= 0, -1 over a sample with ok = 0; out: a contiguous tensor to write into.  One launch, one
    pass.  Exact.  Enqueues only, so it can be captured."""
    name = "homography_residual"
    b, _, h, w = _arg(name, "flow", flow, (torch.float32,), ("B", 2, "h", "w")).shape
    dev = flow.device
    if flow.numel() == 0 or any(s < 0 for s in flow.stride()):
        raise _hip.FocusFlowHipError(f"{name}: flow must be a non-empty (B,2,h,w) without a negative stride, got {tuple(flow.shape)} strides {flow.stride()}")
    _arg(name, "H", H, (torch.float32,), (b, 3, 3), dev, contiguous=True)
    _arg(name, "ok", ok, (torch.uint8,), (b,), dev, contiguous=True)
    out = _out(name, out, (b, h, w), dev)
    _hip.call("ff_homography_residual", _p(flow), *flow.stride(), _p(H), _p(ok), b, h, w, _p(out), _stream())
    return out


_minus_one = {}      # device -> the one-element tensor -1.0 that negate() scales by


def negate(src: Tensor, out: Tensor) -> Tensor:
    """out = -src for two contiguous fp32 tensors of one shape: ff_scale_add_fwd with the scale -1 and no addend (sign flips are
    exact; a zero comes out as +0).  One launch, enqueues only."""
    _arg("negate", "src", src, (torch.float32,), contiguous=True)
    _arg("negate", "out", out, (torch.float32,), tuple(src.shape), src.device, contiguous=True)
    key = src.device
    minus = _minus_one.get(key)
    if minus is None:      # (made once per device, outside any capture: FrameSequence asks for it when it allocates)
        minus = _minus_one[key] = torch.full((1,), -1.0, dtype=torch.float32, device=src.device)
    # mode 1 with B = 1, C = 1: every element is a "pixel" of the one channel whose scale is s[0]
    _hip.call("ff_scale_add_fwd", _p(src), 1, _p(minus), 0, None, None, 0, _p(out), 1, 1, 1, src.numel(), 1, _stream())
    return out


def coords_step(coords1: Tensor, delta: Optional[Tensor], flow4: Optional[Tensor], slot: Optional[Tensor]):
    b, h, w, _ = coords1.shape
    _hip.call("ff_coords_step", _p(coords1), _p(delta), _ld(delta) if delta is not None else 0, _p(flow4), _p(slot),
              _ld(slot) if slot is not None else 0, b, h, w, _stream())


def gru_rh(r: Tensor, h: Tensor, out: Optional[Tensor] = None) -> Tensor:
    b, hh, ww, c = h.shape
    if out is None:
        out = empty_nhwc(b, hh, ww, c, h)
    _hip.call("ff_gru_rh", _p(r), _ld(r), _p(h), _ld(h), _p(out), _ld(out), b * hh * ww, c, _stream())
    return out


def gru_blend(z: Tensor, q: Tensor, h: Tensor, out: Optional[Tensor] = None) -> Tensor:
    b, hh, ww, c = h.shape
    if out is None:
        out = empty_nhwc(b, hh, ww, c, h)
    _hip.call("ff_gru_blend", _p(z), _ld(z), _p(q), _ld(q), _p(h), _ld(h), _p(out), _ld(out), b * hh * ww, c, _stream())
    return out


def gru_pass(direction: int, hs, motion, h: Tensor, zr_pre: Tensor, q_pre: Tensor, wzr_frag: Tensor, wq_frag: Tensor, bzr: Tensor, bq: Tensor,
             w_fmt: int, y: Optional[Tensor] = None, y2: Optional[Tensor] = None, gates=None):
    """One SepConvGRU pass as one launch (ff_gru_pass): hs / motion SplitT, h fp32 -> (h' fp32, h' SplitT).  y / y2: existing
    outputs; gates = (z, r, q) fp32 (B,H,W,128) tensors of one leading dimension: the recorded form (ff_gru_pass_rec) also
    stores what the backward differentiates through."""
    b, hh, ww, c = h.shape
    assert c == 128 and hs.shape == h.shape and motion.shape == h.shape and zr_pre.shape == (b, hh, ww, 256) and q_pre.shape == h.shape
    y = empty_nhwc(b, hh, ww, c, h) if y is None else y
    y2 = empty_nhwc(b, hh, ww, c, h) if y2 is None else y2
    note = (2.0 * b * hh * ww * 384 * 384 * 5, w_fmt)
    # (timed with the convolutions in bench.py's roofline_conv: it IS two of them - 384 -> 256 and 384 -> 128, five taps)
    if gates is None:
        _timed_call("conv", "ff_gru_pass", direction, _p(hs.t), _ld(hs.t), _p(motion.t), _ld(motion.t), _p(h), _ld(h), _p(zr_pre), _ld(zr_pre), _p(q_pre), _ld(q_pre),
                    _p(wzr_frag), _p(wq_frag), _p(bzr), _p(bq), w_fmt, _p(y), _ld(y), _p(y2), _ld(y2), b, hh, ww, _stream(), note=note)
    else:
        z, r, q = gates
        assert z.shape == r.shape == q.shape == h.shape and _ld(z) == _ld(r) == _ld(q)
        _timed_call("conv", "ff_gru_pass_rec", direction, _p(hs.t), _ld(hs.t), _p(motion.t), _ld(motion.t), _p(h), _ld(h), _p(zr_pre), _ld(zr_pre), _p(q_pre), _ld(q_pre),
                    _p(wzr_frag), _p(wq_frag), _p(bzr), _p(bq), w_fmt, _p(y), _ld(y), _p(y2), _ld(y2), _p(z), _p(r), _p(q), _ld(z), b, hh, ww, _stream(), note=note)
    return y, SplitT(y2)


class LazyAct:
    """An activation that exists only as its ingredients: relu(InstanceNorm(t)) after a stem, relu(x + relu(InstanceNorm(t)))
    at the end of a residual stage - `t` raw convolution output, `scale` / `shift` the [B][C] tables of norm_coeffs, `res` the
    block's input or None.  The one consumer that can read it like this is fusion_pair (csrc/fusion_pair.hip: the
    normalisation pass, its write and its re-read disappear); anything else calls materialise() = ff_norm_apply's result,
    bit for bit."""
    __slots__ = ("t", "stats", "count", "eps", "act", "res", "_coef")

    def __init__(self, t: Tensor, stats: Tensor, count: int, eps: float, act: int, res: Optional[Tensor]):
        self.t, self.stats, self.count, self.eps, self.act, self.res, self._coef = t, stats, count, eps, act, res, None

    @property
    def shape(self):
        return self.t.shape

    def coeffs(self):
        if self._coef is None:
            self._coef = norm_coeffs(self.stats, self.count, self.eps)
        return self._coef

    def materialise(self) -> Tensor:
        return norm_apply(self.t, self.stats, True, self.eps, act=self.act, res=self.res, out=self.t)

    def record_stream(self, stream):
        for x in (self.t, self.stats, self.res) + (tuple(self._coef) if self._coef is not None else ()):
            if x is not None:
                x.record_stream(stream)


def fusion_pair_tile(c: int) -> int:
    """Pixels per tile of ff_fusion_pair_fwd for c channels per branch (0: no instance)."""
    return _hip.load().ff_fusion_pair_tile(c)


def fusion_pair_inputs_ok(*ins) -> bool:
    """ff_fusion_pair_fwd reads contiguous NHWC tensors (leading dimension == C) of less than 2 GiB."""
    for v in ins:
        for t in ((v.t, v.res) if isinstance(v, LazyAct) else (v,)):
            if t is not None and (not t.is_cuda or _ld(t) != t.shape[3] or t.numel() * 4 >= (1 << 31)):
                return False
    return True


def fusion_pair(img, mask, w_frag, bias, w_fmt: int):
    """FusionUnit '1x1conv', both directions, one launch (ff_fusion_pair_fwd): img / mask fp32 NHWC tensors or LazyAct;
    w_frag = (mask2img, img2mask) weights in fragment order, bias likewise -> (img', mask')."""
    ins = (img, mask)
    b, h, w, c = ins[0].shape
    assert ins[1].shape == ins[0].shape
    p = _hip.FFFusionPair()
    outs = []
    for i, v in enumerate(ins):
        t = v.t if isinstance(v, LazyAct) else v
        _require_gpu(t)
        p.x[i], p.x_ld[i] = t.data_ptr(), _ld(t)
        if isinstance(v, LazyAct):
            sc, sh = v.coeffs()
            p.scale[i], p.shift[i] = sc.data_ptr(), sh.data_ptr()
            p.in_act = v.act
            if v.res is not None:
                p.xres[i], p.xres_ld[i] = v.res.data_ptr(), _ld(v.res)
        y = t if isinstance(v, LazyAct) else empty_nhwc(b, h, w, c, t)       # a lazy input's raw tensor has no other reader: write over it
        outs.append(y)
        p.y[i], p.y_ld[i] = y.data_ptr(), _ld(y)
        p.w_frag[i] = w_frag[i].data_ptr()
        p.bias[i] = bias[i].data_ptr() if bias[i] is not None else None
    if _range_word is not None:      # CHECK_RANGE: what the unit reads goes through the split format like any convolution input
        for v in ins:
            # (a lazy value is relu(res + relu(InstanceNorm(t))): bounded by the residual, which is probed; t itself never meets the format)
            probe = v.res if isinstance(v, LazyAct) else v
            if probe is not None:
                _range_probe(probe)
    acts = {v.act for v in ins if isinstance(v, LazyAct)}
    assert len(acts) <= 1, "lazy inputs of one fusion unit share the activation"
    p.w_format, p.B, p.HW, p.C = w_fmt, b, h * w, c
    # (timed with the convolutions in bench.py's roofline_conv: two C x C 1x1 convolutions)
    _timed_call("conv", "ff_fusion_pair_fwd", C.byref(p), _stream(), note=(2.0 * b * h * w * 2 * c * c, w_fmt))
    return outs[0], outs[1]


def encoder_tail_inputs_ok(*ins) -> bool:
    """ff_encoder_tail_fwd reads two contiguous NHWC tensors of 128 channels (fp32 or LazyAct) on the device; its 256-channel
    output stays below 2 GiB."""
    if not fusion_pair_inputs_ok(*ins) or ins[0].shape != ins[1].shape:
        return False
    b, h, w, c = ins[0].shape
    return c == 128 and b * h * w * 256 * 4 < (1 << 31) and all((v.t if isinstance(v, LazyAct) else v).dtype == torch.float32 for v in ins)


def encoder_tail(x, m, w_frag: Tensor, bias: Tensor, w_fmt: int) -> Tensor:
    """The output stage of a CCE encoder - fusion4, conv2 / mask_conv2, fusion5 - as ONE launch (ff_encoder_tail_fwd):
    x / m the two stage-3 outputs (fp32 NHWC, 128 channels, or LazyAct); w_frag the composed 256 x 256 weight over the segments
    [x | m] in fragment order, bias [256] -> (B, H, W, 256).  What the kernel cannot read is refused by the library."""
    ins = (x, m)
    b, h, w, c = ins[0].shape
    p = _hip.FFEncoderTail()
    for i, v in enumerate(ins):
        t = v.t if isinstance(v, LazyAct) else v
        _require_gpu(t)
        if tuple(t.shape[:3]) != (b, h, w):
            raise _hip.FocusFlowHipError(f"encoder_tail: inputs of different shapes {tuple(ins[0].shape)} / {tuple(t.shape)}")
        c = min(c, t.shape[3])
        p.x[i], p.x_ld[i] = t.data_ptr(), _ld(t)
        if isinstance(v, LazyAct):
            sc, sh = v.coeffs()
            p.scale[i], p.shift[i] = sc.data_ptr(), sh.data_ptr()
            p.in_act = v.act
            if v.res is not None:
                p.xres[i], p.xres_ld[i] = v.res.data_ptr(), _ld(v.res)
    acts = {v.act for v in ins if isinstance(v, LazyAct)}
    assert len(acts) <= 1, "lazy inputs of one stage share the activation"
    if _range_word is not None:      # CHECK_RANGE: as fusion_pair - a lazy value is bounded by its residual
        for v in ins:
            probe = v.res if isinstance(v, LazyAct) else v
            if probe is not None:
                _range_probe(probe)
    _require_gpu(bias)
    cout = bias.numel()
    y = empty_nhwc(b, h, w, cout, bias)
    p.w_frag, p.bias, p.w_format = w_frag.data_ptr(), bias.data_ptr(), w_fmt
    p.y, p.y_ld = y.data_ptr(), cout
    p.B, p.HW, p.C, p.Cout = b, h * w, c, cout
    # (timed with the convolutions in bench.py's roofline_conv: one 2C -> Cout 1x1 convolution, the FLOP the kernel issues)
    _timed_call("conv", "ff_encoder_tail_fwd", C.byref(p), _stream(), note=(2.0 * b * h * w * 2 * c * cout, w_fmt))
    return y


def conv_s2_pair_stats_parts(h: int, w: int) -> int:
    """Statistics entries per (image, channel) of ff_conv_s2_pair_fwd over an h x w input: one per 4 x 16 output tile."""
    return _hip.load().ff_conv_s2_pair_stats_parts(h, w)


def conv_s2_pair_inputs_ok(x, cout: int) -> bool:
    """ff_conv_s2_pair_fwd reads one fp32 NHWC tensor (a channel slice too) of a multiple of 32 channels, 16-byte aligned,
    below 2 GiB, and writes 96 or 128 channels."""
    if not isinstance(x, Tensor) or x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32:
        return False
    b, h, w, c = x.shape
    if c % 32 or cout not in (96, 128) or x.stride(3) != 1 or x.data_ptr() % 16 or b >= 65536:
        return False
    ld = x.stride(2) if w > 1 else (x.stride(1) if h > 1 else max(x.stride(0), c))
    if ld % 4 or ld < c or (w > 1 and h > 1 and x.stride(1) != w * ld) or (b > 1 and x.stride(0) != h * w * ld):
        return False
    return b * h * w * ld * 4 < (1 << 31)


def conv_s2_pair(x: Tensor, w3_frag: Tensor, w1_frag: Tensor, bias3: Optional[Tensor], bias1: Optional[Tensor], cout: int, w_fmt: int,
                 scale=(None, None), shift=(None, None), act=(ACT_NONE, ACT_NONE), want_stats: bool = False, out=(None, None),
                 kernels=((3, 2, 1), (1, 2, 0))):
    """The entry of a stride-2 residual block as ONE launch (ff_conv_s2_pair_fwd): a = conv3x3(x), stride 2, pad 1 and
    d = conv1x1(x), stride 2, pad 0 from one pass over x; w3_frag / w1_frag the two weights in fragment order (PackedConv.frag),
    scale / shift / act per output (a folded eval BatchNorm) -> (a, d), or - want_stats - (a, stats_a, d, stats_d) with the
    per-sample {sum, sum of squares} tables of norm_stats, from the launch's own epilogue.  `kernels`: (size, stride, pad) of the
    two convolutions; what the kernel cannot read is refused by the library."""
    _require_gpu(x)
    b, h, w, cin = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    p = _hip.FFConvS2Pair()
    p.x, p.x_ld = x.data_ptr(), _ld(x)
    p.B, p.H, p.W, p.Cin, p.Cout = b, h, w, cin, cout
    for i, (k, s, pd) in enumerate(kernels):
        p.k[i], p.stride[i], p.pad[i] = k, s, pd
    p.w3_frag, p.w1_frag, p.w_format = w3_frag.data_ptr(), w1_frag.data_ptr(), w_fmt
    outs, parts = [], []
    nparts = conv_s2_pair_stats_parts(h, w) if want_stats else 0
    for i, bias in enumerate((bias3, bias1)):
        y = out[i] if out[i] is not None else empty_nhwc(b, ho, wo, cout, x)
        assert tuple(y.shape) == (b, ho, wo, cout)
        outs.append(y)
        p.y[i], p.y_ld[i] = y.data_ptr(), _ld(y)
        p.bias[i] = bias.data_ptr() if bias is not None else None
        if scale[i] is not None:
            p.scale[i], p.shift[i] = scale[i].data_ptr(), shift[i].data_ptr()
        p.act[i] = act[i]
        if nparts:
            parts.append(torch.empty(b * nparts * cout * 4, dtype=torch.float32, device=x.device))
            p.stats_part[i] = parts[i].data_ptr()
    if _range_word is not None:      # CHECK_RANGE: x goes through the split format like any convolution input
        _range_probe(x)
    # (timed with the convolutions in bench.py's roofline_conv: the useful FLOP of both convolutions)
    _timed_call("conv", "ff_conv_s2_pair_fwd", C.byref(p), _stream(), note=(2.0 * b * ho * wo * cout * cin * 10, w_fmt))
    if not want_stats:
        return outs[0], outs[1]
    stats = []
    for i in range(2):
        st = _zero_stats(b, cout, x.device)
        _hip.call("ff_norm_stats_finish", _p(parts[i]), b, nparts, cout, _p(st), _stream())
        stats.append(st)
    return outs[0], stats[0], outs[1], stats[1]


def mask_upsample_pack(w_split: Tensor) -> Tensor:
    """Split rows of the mask head's second convolution (576 x 256) -> ff_mask_upsample_fwd's stage-major weight image."""
    assert w_split.dtype == torch.uint8 and w_split.numel() == 576 * 1024 and w_split.is_contiguous()
    out = torch.empty_like(w_split)
    _hip.call("ff_mask_upsample_pack", _p(w_split), _p(out), _stream())
    return out


def mask_upsample(hid: Tensor, w_stage: Tensor, w_fmt: int, bias: Optional[Tensor], flow: Tensor, out_scale: float = 0.25) -> Tensor:
    """mask[2] (1x1, 256 -> 576) * out_scale + soft-max + convex up-sampling in one launch (ff_mask_upsample_fwd).
    hid: (B,H,W,256) view of the mask head's hidden tensor; w_stage: mask_upsample_pack(split rows); flow: (B,H,W,>=2).
    -> (B,2,8H,8W)."""
    b, h, w, c = hid.shape
    assert c == 256 and w_fmt in (_hip.W_F16X3, _hip.W_F16) and flow.shape[:3] == (b, h, w)
    out = torch.empty((b, 2, 8 * h, 8 * w), dtype=torch.float32, device=hid.device)
    _hip.call("ff_mask_upsample_fwd", _p(hid), _ld(hid), _p(w_stage), w_fmt, _p(bias), out_scale, _p(flow), _ld(flow), _p(out), b, h, w, _stream())
    return out


def upsample_flow(flow: Tensor, mask: Tensor) -> Tensor:
    """flow (B,H,W,>=2) NHWC, mask (B,H,W,576) NHWC -> (B,2,8H,8W) NCHW."""
    b, h, w, _ = flow.shape
    out = torch.empty((b, 2, 8 * h, 8 * w), dtype=torch.float32, device=flow.device)
    _hip.call("ff_upsample_flow", _p(flow), _ld(flow), _p(mask), _ld(mask), _p(out), b, h, w, _stream())
    return out


def nhwc_to_nchw(x: Tensor) -> Tensor:
    b, h, w, c = x.shape
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=x.device)
    _hip.call("ff_nhwc_to_nchw", _p(x), _ld(x), _p(out), b, h, w, c, _stream())
    return out


# ----------------------------------------------------------------------------
# backward wrappers
# ----------------------------------------------------------------------------
def _conv_params(xs, b, h, w, cout, kh, kw, stride, pad, ho, wo, dilation=1):
    p = FFConvParams()
    p.dil_h = p.dil_w = dilation
    for i, x in enumerate(xs):
        p.x[i], p.x_ld[i], p.x_c[i], p.x_gstride[i] = x.data_ptr(), _ld(x), x.shape[3], 0
    p.groups, p.B, p.H, p.W = 1, b, h, w
    p.Ho, p.Wo, p.Cout = ho, wo, cout
    p.KH, p.KW, p.stride, p.pad_h, p.pad_w = kh, kw, stride, pad[0], pad[1]
    p.out_scale = 1.0
    return p


def conv2d_wgrad(xs: Sequence[Tensor], g: Tensor, cout: int, kh: int, kw: int, stride: int, pad,
                 g_amax: Optional[Tensor] = None, want_db: bool = False, dw: Optional[Tensor] = None,
                 db: Optional[Tensor] = None, dilation: int = 1):
    """packed dW [cout][kh*kw*cin] from inputs `xs` and output gradient g (B,Ho,Wo,>=cout, ld % 4 == 0).
    With g_amax (bits of max|g|, act_bwd) and a split conv format the kernel runs on the f16 matrix pipe and can
    also return the bias gradient: -> dW, or (dW, db) when want_db.  `dw` / `db`: existing buffers to ADD into
    (the kernel accumulates with atomics; fresh zeroed ones are allocated when omitted)."""
    b, h, w, _ = xs[0].shape
    _, ho, wo, _ = g.shape
    cin = sum(x.shape[3] for x in xs)
    if dw is None:
        dw = torch.zeros((cout, kh * kw * cin), dtype=torch.float32, device=g.device)
    assert dw.shape == (cout, kh * kw * cin) and dw.is_contiguous()
    p = _conv_params(xs, b, h, w, cout, kh, kw, stride, pad, ho, wo, dilation)
    p.y, p.y_ld = g.data_ptr(), _ld(g)
    fmt = w_format() if g_amax is not None else 0
    if fmt:
        p.w_format, p.x_amax = fmt, g_amax.data_ptr()
        if want_db and db is None:
            db = torch.zeros(cout, dtype=torch.float32, device=g.device)
    else:
        assert db is None, "accumulating bias-gradient buffers need a split conv format"
    _hip.call("ff_conv2d_wgrad", C.byref(p), _p(dw), 0, _p(db) if fmt else None, _stream())
    if want_db:
        return dw, (db if db is not None else channel_sum(g, cout))
    return dw


def unpack_conv_wgrad(packed: Tensor, cout, cin, kh, kw, cin_pad, cout_offset) -> Tensor:
    dw = torch.empty((cout, cin, kh, kw), dtype=torch.float32, device=packed.device)
    _hip.call("ff_unpack_conv_wgrad", _p(packed), cout, cin, kh, kw, cin_pad, cout_offset, _p(dw), _stream())
    return dw


def pack_weights_table(table_dev: Tensor, njobs: int, total_blocks: int):
    """Run a device-resident FFPackJob table (cce.prepack builds it): every stale weight layout in one launch."""
    if not table_dev.is_cuda:
        raise _hip.FocusFlowHipError("ff_pack_weights_table: the job table must live on the HIP device")
    _hip.call("ff_pack_weights_table", _p(table_dev), njobs, total_blocks, _stream())


def unpack_wgrad_group(dw: Tensor, db: Optional[Tensor], couts, offs, has_bias, cin_src: int, slices, kh: int, kw: int,
                       cin_pad: int) -> Tensor:
    """Packed dW rows (+ db) of one PackedConv -> one flat tensor: per member its OIHW gradient (zero outside `slices`),
    then its bias gradient if has_bias[m]."""
    _require_gpu(dw)
    n = len(couts)
    total = sum(c * cin_src * kh * kw + (c if hb else 0) for c, hb in zip(couts, has_bias))
    out = torch.empty(total, dtype=torch.float32, device=dw.device)
    arr = C.c_int * n
    ns = len(slices) if slices else 0
    sarr = C.c_int * max(ns, 1)
    _hip.call("ff_unpack_wgrad_group", _p(dw), _p(db), n, arr(*couts), arr(*offs), arr(*[int(bool(h)) for h in has_bias]), cin_src, ns,
              sarr(*([lo for lo, _ in slices] if ns else [0])), sarr(*([hi for _, hi in slices] if ns else [0])), kh, kw, cin_pad,
              _p(out), _stream())
    return out


def pack_conv_weight_dgrad(w_oihw: Tensor, dst: Tensor, cout_pad: int, cout_offset: int):
    co, ci, kh, kw = w_oihw.shape
    # rows beyond Cin (channel padding of the forward input) stay zero: their input gradient is zero
    assert dst.is_contiguous() and dst.shape[0] >= ci and dst.shape[1] == kh * kw * cout_pad
    _hip.call("ff_pack_conv_weight_dgrad", _p(w_oihw.contiguous()), co, ci, kh, kw, _p(dst), cout_pad, cout_offset, _stream())


def act_bwd(dy: Tensor, y: Optional[Tensor], act: int, scale: float, c: int, want_amax: bool = False,
            amax: Optional[Tensor] = None):
    """g = dy*act'(y)*scale over the first c channels, zero-padded to a multiple of 4.
    want_amax: also return a device word with the bits of max|g| (-> conv2d(x_amax=...)); `amax`: a zeroed int32
    word to use for it instead of allocating one."""
    b, h, w, _ = dy.shape
    cpad = (c + 3) // 4 * 4
    # no activation, no scale, nothing to pad: g IS dy (ff_act_bwd with g == dy only measures max|dy|, no copy)
    alias = act == ACT_NONE and scale == 1.0 and dy.shape[3] == c == cpad and _ld(dy) == cpad and dy.data_ptr() % 16 == 0
    g = dy if alias else empty_nhwc(b, h, w, cpad, dy)
    if alias and not want_amax:
        return g
    if want_amax and amax is None:
        amax = torch.zeros(1, dtype=torch.int32, device=dy.device)
    _hip.call("ff_act_bwd", _p(dy), _ld(dy), _p(y), _ld(y) if y is not None else 0, _p(g), cpad, b * h * w, c, cpad,
              act, scale, _p(amax), _stream())
    return (g, amax) if want_amax else g


def act_bwd_into(dy: Tensor, y: Optional[Tensor], act: int, g: Tensor, amax: Tensor, scale: float = 1.0):
    """ff_act_bwd into an existing gradient tensor g (same channel count as dy, a multiple of 4), max|g| into the zeroed
    word `amax` (the recorded update loop: train_loop.py)."""
    b, h, w, c = dy.shape
    assert g.shape == dy.shape and c % 4 == 0
    _hip.call("ff_act_bwd", _p(dy), _ld(dy), _p(y), _ld(y) if y is not None else 0, _p(g), _ld(g), b * h * w, c, c, act, scale, _p(amax), _stream())
    return g


def deconv4x4s2_small(x: Tensor, w_rows: Tensor, bias: Optional[Tensor], cout: int, out: Tensor) -> Tensor:
    """ConvTranspose2d(Cin, cout <= 2, 4, 2, 1) of NHWC x (B,H,W,Cin) into `out` (B,2H,2W,>=cout) - ff_deconv4x4s2_small.
    w_rows: fp32 rows [cout][16*Cin] of the equivalent forward conv (transposed + flipped parameter, pack_conv_weight)."""
    b, h, w, cin = x.shape
    assert out.shape[:3] == (b, 2 * h, 2 * w) and w_rows.shape == (cout, 16 * cin) and w_rows.dtype == torch.float32
    _hip.call("ff_deconv4x4s2_small", _p(x), _ld(x), b, h, w, cin, _p(w_rows), _p(bias), cout, _p(out), _ld(out), _stream())
    return out


def dilate2(g: Tensor, hd: int, wd: int) -> Tensor:
    b, ho, wo, c = g.shape
    out = empty_nhwc(b, hd, wd, c, g)
    _hip.call("ff_dilate2", _p(g), _ld(g), _p(out), b, ho, wo, hd, wd, c, _stream())
    return out


def channel_sum(g: Tensor, c: int) -> Tensor:
    """sum over pixels of the first c channels (bias gradient); fp64 accumulation in ff_norm_stats."""
    b, h, w, cp = g.shape
    outs = []
    for lo in range(0, c, 256):          # ff_norm_stats handles <= 256 channels per call
        hi = min(cp, lo + 256)
        st = norm_stats(g[..., lo:hi], per_sample=False)
        outs.append(st[0, :, 0])
    return torch.cat(outs)[:c].float()


def act_bwd_is_alias(dy: Tensor, act: int, scale: float, c: int) -> bool:
    """act_bwd's no-copy case: no activation, no scale, nothing to pad - the conv's gradient IS dy."""
    return act == ACT_NONE and scale == 1.0 and dy.shape[3] == c == (c + 3) // 4 * 4 and _ld(dy) == c and dy.data_ptr() % 16 == 0


def norm_bwd(x, dy, y, fstats, per_sample, fixed_stats, eps, gamma, beta, relu, want_dres, amax: Optional[Tensor] = None,
             bstats: Optional[Tensor] = None):
    """amax: a zeroed int32 word that receives the bits of max|dx| (saves the consumer conv's measuring pass);
    bstats: a zeroed fp64 (S, C, 2) buffer for the two backward sums (allocated here when omitted)."""
    b, h, w, c = x.shape
    if bstats is None:
        bstats = torch.zeros((b if per_sample else 1, c, 2), dtype=torch.float64, device=x.device)
    assert bstats.shape == (b if per_sample else 1, c, 2) and bstats.dtype == torch.float64
    dx = empty_nhwc(b, h, w, c, x)
    dres = empty_nhwc(b, h, w, c, x) if want_dres else None
    _hip.call("ff_norm_bwd", _p(x), _ld(x), _p(dy), _ld(dy), _p(y), _ld(y) if y is not None else 0, _p(fstats),
              _p(bstats), int(per_sample), int(fixed_stats), eps, _p(gamma), _p(beta), int(relu), _p(dx), c,
              _p(dres), c if want_dres else 0, b, h * w, c, _p(amax), _stream())
    return dx, dres, bstats


def corr_lookup_tiled_bwd(dpyr: TiledPyramid, coords: Tensor, dout: Tensor):
    """Scatter d(lookup output) into the tiled fp32 gradient planes (accumulates)."""
    b, h, w, _ = coords.shape
    assert not dpyr.half
    _hip.call("ff_corr_lookup_tiled_bwd", dpyr.ptrs(), _p(coords), _p(dout), _ld(dout), b * h * w, dpyr.h0, dpyr.w0, _stream())


LOOKUP_BWD_ALL_MAX = 32      # csrc/corr_lookup_tiled.hip: LBA_MAXT


def lookup_bwd_all_fits(h0: int, w0: int) -> bool:
    """Whether ff_corr_lookup_tiled_bwd_all takes planes of this size (the four gradient planes of a query in 64 KB of LDS)."""
    return sum((h0 >> l) * (w0 >> l) for l in range(4)) * 4 <= 64 * 1024


def corr_lookup_tiled_bwd_all(coords_list, dout_list, h0: int, w0: int):
    """d(volume) [B*Q][plane_0] (tiled fp32) from every lookup of a pass at once (ff_corr_lookup_tiled_bwd_all), or None
    when the kernel declines (planes too large for LDS, more than 32 lookups): the caller then goes launch by launch."""
    n = len(coords_list)
    b, h, w, _ = coords_list[0].shape
    q = b * h * w
    ld = _ld(dout_list[0])
    assert all(c.is_contiguous() and c.shape == (b, h, w, 2) for c in coords_list) and all(_ld(d) == ld for d in dout_list)
    d0 = torch.empty((q, TiledPyramid.plane_elems(h0, w0, 0, False)), dtype=torch.float32, device=coords_list[0].device)
    cl = (C.c_void_p * n)(*[c.data_ptr() for c in coords_list])
    dl = (C.c_void_p * n)(*[d.data_ptr() for d in dout_list])
    lib = _hip.load()
    rc = lib.ff_corr_lookup_tiled_bwd_all(_p(d0), cl, dl, n, ld, q, h0, w0, _stream())
    if rc == 1:
        return None
    if rc != 0:
        raise _hip.FocusFlowHipError(f"ff_corr_lookup_tiled_bwd_all failed ({rc}): {lib.ff_last_error().decode()}")
    return d0


def corr_pyramid_tiled_bwd(dpyr: TiledPyramid):
    """avg_pool2d backward chain, in place: afterwards dpyr.levels[0] is d(volume) in tile order."""
    lv = dpyr.levels
    _hip.call("ff_corr_pyramid_tiled_bwd", _p(lv[0]), _p(lv[1]), _p(lv[2]), _p(lv[3]), lv[0].shape[0], dpyr.h0, dpyr.w0, _stream())


def corr_tile_rows(x: Tensor, h: int, w: int, to_tiled: bool) -> Tensor:
    """(B, Q, C) feature rows <-> (B, P, C) rows in the tile order of a level-0 plane (pad rows zero)."""
    b, n, c = x.shape
    p = TiledPyramid.plane_elems(h, w, 0, False)
    assert x.is_contiguous() and n == (h * w if to_tiled else p)
    out = torch.empty((b, p if to_tiled else h * w, c), dtype=torch.float32, device=x.device)
    _hip.call("ff_corr_tile_rows", _p(x), _p(out), b, h, w, c, int(to_tiled), _stream())
    return out


def grouped_1x1(x: Tensor, wt: Tensor, out_scale: float) -> Tensor:
    """y[g] = x[g] (M x K) @ wt[g]^T (N x K)^T * out_scale, all contiguous (G, M, K), (G, N, K)."""
    g, m, k = x.shape
    n = wt.shape[1]
    y = torch.empty((g, m, n), dtype=torch.float32, device=x.device)
    p = FFConvParams()
    p.x[0], p.x_ld[0], p.x_c[0], p.x_gstride[0] = x.data_ptr(), k, k, m * k
    p.groups, p.B, p.H, p.W = g, 1, 1, m
    p.w, p.w_gstride = wt.data_ptr(), n * k
    p.out_scale = out_scale
    p.y, p.y_ld, p.y_gstride = y.data_ptr(), n, m * n
    p.Ho, p.Wo, p.Cout = 1, m, n
    p.KH = p.KW = p.stride = 1
    _require_gpu(x)
    _hip.call("ff_conv2d_fwd", C.byref(p), _stream())
    return y


def corr_volume_bwd(dvol: Tensor, f1: Tensor, f2: Tensor, tiled: bool = False):
    """BmmBackward of corr.py:58: df1 = dvol @ f2 / sqrt(C), df2 = dvol^T @ f1 / sqrt(C).
    tiled: dvol is (B, Q, P) with the fmap2 index j in the tile order of a level-0 plane (pad columns zero): the
    contraction over j runs over fmap2's rows gathered into the same order, and df2's rows are un-permuted at the end."""
    b, h, w, c = f1.shape
    q = h * w
    s = 1.0 / math.sqrt(c)
    if tiled:
        qn = dvol.shape[-1]
        dvol = dvol.contiguous().view(b, q, qn)
        f2r = corr_tile_rows(f2.contiguous().view(b, q, c), h, w, True)        # (B, P, C), pad rows zero
        qp = qn
    else:
        qn = q
        dvol = dvol.contiguous().view(b, q, q)
        qp = (q + 3) // 4 * 4
        if qp != q:      # odd plane sizes: the kernels read the contraction index in 16-byte groups -> zero-pad its rows
            dvol = torch.nn.functional.pad(dvol, (0, qp - q))
        f2r = f2.contiguous().view(b, q, c)
    if qp == qn:
        f2t = f2r.transpose(1, 2).contiguous()                                    # [c][j] = f2[j][c]: one launch for the batch
    else:
        f2t = torch.zeros((b, c, qp), dtype=torch.float32, device=f1.device)
        for i in range(b):
            _hip.call("ff_pack_conv_weight_dgrad", _p(f2r[i]), qn, c, 1, 1, _p(f2t[i]), qp, 0, _stream())
    df1 = grouped_1x1(dvol, f2t, s).view(b, h, w, c)
    df2 = torch.zeros((b, qn, c), dtype=torch.float32, device=f1.device)
    p = FFConvParams()
    p.x[0], p.x_ld[0], p.x_c[0], p.x_gstride[0] = f1.data_ptr(), c, c, q * c
    p.groups, p.B, p.H, p.W = b, 1, 1, q
    p.Ho, p.Wo, p.Cout = 1, q, qn
    p.KH = p.KW = p.stride = 1
    p.out_scale = s
    p.y, p.y_ld, p.y_gstride = dvol.data_ptr(), qp, q * qp
    _hip.call("ff_conv2d_wgrad", C.byref(p), _p(df2), qn * c, None, _stream())
    if tiled:
        df2 = corr_tile_rows(df2, h, w, False)
    return df1, df2.view(b, h, w, c)


def gru_rh_bwd(drh, r, h):
    b, hh, ww, c = h.shape
    dr, dh = empty_nhwc(b, hh, ww, c, h), empty_nhwc(b, hh, ww, c, h)
    _hip.call("ff_gru_rh_bwd", _p(drh), _ld(drh), _p(r), _ld(r), _p(h), _ld(h), _p(dr), c, _p(dh), c, b * hh * ww, c, _stream())
    return dr, dh


def gru_blend_bwd(dhn, z, q, h):
    b, hh, ww, c = h.shape
    dz, dq, dh = (empty_nhwc(b, hh, ww, c, h) for _ in range(3))
    _hip.call("ff_gru_blend_bwd", _p(dhn), _ld(dhn), _p(z), _ld(z), _p(q), _ld(q), _p(h), _ld(h), _p(dz), c, _p(dq), c,
              _p(dh), c, b * hh * ww, c, _stream())
    return dz, dq, dh


def upsample_flow_bwd(dout: Tensor, flow: Tensor, mask: Tensor):
    b, h, w, _ = flow.shape
    dflow = torch.zeros((b, h, w, 2), dtype=torch.float32, device=flow.device)
    dmask = empty_nhwc(b, h, w, 576, flow)
    _hip.call("ff_upsample_flow_bwd", _p(dout.contiguous()), _p(flow), _ld(flow), _p(mask), _ld(mask), _p(dflow), _p(dmask),
              b, h, w, _stream())
    return dflow, dmask
