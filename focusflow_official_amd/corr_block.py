"""CorrBlock on the HIP path (corr.py:12-60): all-pairs volume on the f16 matrix pipe (fp16-split operands, fp32-level
accuracy) with the 4-level average-pool pyramid written once from the accumulators in a tiled HBM layout, and the
radius-4 bilinear window lookup over that layout."""
import functools
import os

import torch

from . import _hip, fn, ops

PYRAMID_DTYPES = ("fp32", "fp16")
_MAX_PYRAMID_BYTES = int(os.environ.get("FF_MAX_PYRAMID_BYTES", str(3900 * 1000 * 1000)))      # (tests lower it to exercise the chunking)
_LOOKUP_SPAN = 0xfff00000      # csrc/corr_lookup_dma.hip: the four levels of a lookup lie within this many bytes (one buffer resource)
_LOOKUP_BWD_ALL = True   # one lookup-backward launch per pass instead of one per iteration (tests switch it off)


@functools.lru_cache(maxsize=64)
def pyramid_span(h: int, w: int, half: bool, pairs: int = 1) -> int:
    """Bytes from the first to the last element of the four levels of `pairs` pyramids as ops.TiledPyramid.empty lays them out."""
    esz = 2 if half else 4
    n = [pairs * h * w * ops.TiledPyramid.plane_elems(h, w, l, half) for l in range(4)]
    return sum((x * esz + 255) // 256 * 256 for x in n[:3]) + n[3] * esz


def pyramid_bytes(b: int, h: int, w: int, half: bool) -> int:
    """Bytes of the materialised pyramid of a batch of b pairs at h x w (1/8 resolution)."""
    return b * h * w * sum(ops.TiledPyramid.plane_elems(h, w, l, half) for l in range(4)) * (2 if half else 4)


def pyramid_fits(b: int, h: int, w: int, pyramid_dtype: str = None) -> bool:
    """Whether a RECORDED pass can materialise the batch's pyramid: one allocation under _MAX_PYRAMID_BYTES (a recorded
    pass keeps one pyramid for its backward) and one pair within the lookup's buffer resource."""
    half = (pyramid_dtype or os.environ.get("FF_CORR_PYRAMID", "fp32")) == "fp16"
    return pyramid_bytes(b, h, w, half) < _MAX_PYRAMID_BYTES and pyramid_span(h, w, half) < _LOOKUP_SPAN


class _Block:
    """What the two correlation blocks share.  The reference's call protocol: build once per pair, then
    ``__call__(coords, want_taps=False)`` per iteration with NHWC (B, H8, W8, 2) [x, y] coordinates -> NHWC (B, H8, W8, 324)
    (+ int32 taps (B*H8*W8, 4, 2, 9)).  A block provides ``build(fmap1, fmap2)``, ``lookup(coords, out=None, want_taps=False)``
    (plain launches, no autograd) and its gradient side: ``grad_add(coords, dout)`` per lookup, then once per pass
    ``grad_finish(fmap1, fmap2) -> (d fmap1, d fmap2)``, which resets it.  Recorded feature maps: fn.CorrBuildFn /
    fn.LookupFn drive them; a block built outside the tape (``fusable``) is driven by the fused update-loop node
    (train_loop.UpdateLoopFn) itself."""
    _token = None       # recorded feature maps: the token of the build's autograd node (fn.CorrBuildFn)
    _chunks = None      # CorrBlock in batch chunks: [(lo, hi, CorrBlock of pairs lo .. hi-1)]

    def __init__(self, num_levels: int, radius: int):
        if num_levels != 4 or radius != 4:
            raise NotImplementedError("the correlation kernels are built for 4 levels, radius 4 (all reference configs)")
        self.num_levels, self.radius = num_levels, radius
        self._nk = num_levels * (2 * radius + 1) ** 2
        self._padded = None
        self.pending = []

    def _build_or_record(self, fmap1: torch.Tensor, fmap2: torch.Tensor):
        fmap1, fmap2 = fmap1.contiguous(), fmap2.contiguous()
        if fn.recording(fmap1, fmap2):
            self._token = fn.CorrBuildFn.apply(fmap1, fmap2, self)      # (its forward builds the block)
        else:
            self.build(fmap1, fmap2)

    @property
    def fusable(self) -> bool:
        """Whether the fused update-loop node can take the block: built outside the tape (the node differentiates through
        it itself), one pyramid or operand set."""
        return self._token is None and self._chunks is None

    def __call__(self, coords: torch.Tensor, want_taps: bool = False):
        if self._token is not None and not want_taps:
            return fn.LookupFn.apply(self._token, self, coords)
        if want_taps or torch.is_grad_enabled():
            # a fresh tensor per call: a recorded update block saves its input (convc1's weight gradient), which the next
            # iteration's lookup would overwrite in a shared buffer
            return self.lookup(coords, want_taps=want_taps)
        # Inference: the lookup writes into a buffer whose channel count is padded to a multiple of 32 (324 -> 352, pad
        # channels zero once), so that convc1 takes the block-uniform loader (32-channel chunks) of the conv kernel instead
        # of the generic im2col one.  The buffer is reused by every iteration of this pair.
        if self._padded is None:
            b, h, w, _ = coords.shape
            self._padded = torch.zeros((b, h, w, (self._nk + 31) // 32 * 32), dtype=torch.float32, device=coords.device)
        self.lookup(coords, out=self._padded[..., :self._nk])
        return self._padded


class CorrBlock(_Block):
    """The reference's CorrBlock.  fmap1/fmap2: NHWC (B, H8, W8, C) fp32.  HBM layout: ops.TiledPyramid (128-byte 2-D tiles
    per plane).  ``pyramid_dtype``: "fp32" (default; the reference's arithmetic) or "fp16" (storage only: every level is
    rounded to half after it has been computed in fp32 from the stored level below, as torch autocast would - BASELINE
    configs[4]; the lookup still interpolates in fp32).  ``corr_pyramid`` gives the levels back as row-major fp32 planes.
    The backward accumulates into tiled fp32 gradient planes (no per-iteration volume-sized buffers), folds them down the
    pooling chain to d(volume) and contracts that with the feature maps (BmmBackward of corr.py:58); fp16 storage is a
    straight-through rounding for the gradient, as a cast under autocast would be."""

    def __init__(self, fmap1: torch.Tensor, fmap2: torch.Tensor, num_levels: int = 4, radius: int = 4,
                 pyramid_dtype: str = None):
        super().__init__(num_levels, radius)
        pyramid_dtype = pyramid_dtype or os.environ.get("FF_CORR_PYRAMID", "fp32")
        if pyramid_dtype not in PYRAMID_DTYPES:
            raise ValueError(f"pyramid_dtype must be one of {PYRAMID_DTYPES}")
        self.half = pyramid_dtype == "fp16"
        self.pyr = self.grad_pyr = None
        fmap1, fmap2 = fmap1.contiguous(), fmap2.contiguous()
        b, h, w, _ = fmap1.shape
        if fmap1.is_cuda and pyramid_span(h, w, self.half) >= _LOOKUP_SPAN:
            # refused before the pyramid is allocated and built (the lookup would refuse it afterwards)
            fits16 = not self.half and pyramid_span(h, w, True) < _LOOKUP_SPAN
            raise _hip.FocusFlowHipError(
                f"CorrBlock: the {pyramid_dtype} correlation pyramid of ONE pair at {h}x{w} (1/8 resolution) spans "
                f"{pyramid_span(h, w, self.half) / 1e9:.2f} GB; the lookup addresses a pyramid through one 4 GB buffer resource.  "
                "Use alternate_corr=True (on-the-fly correlation, memory linear in the image area)"
                + (', or corr_pyramid_dtype="fp16" (its pyramid fits)' if fits16 else "") + ".")
        # The lookup kernel addresses the four levels of a pyramid through ONE buffer resource (32-bit byte offsets): a batch
        # whose pyramid would pass 4 GB - configs[4] beyond 22 pairs: 177 MB of fp16 planes per pair - is built and looked up
        # in batch chunks, each with its own allocation (inference; a recorded pass keeps one pyramid for its backward).
        per_pair = pyramid_bytes(1, h, w, self.half) if fmap1.is_cuda else 0
        if per_pair * b >= _MAX_PYRAMID_BYTES and b > 1 and not fn.recording(fmap1, fmap2):
            per = max(1, _MAX_PYRAMID_BYTES // per_pair)
            self._chunks = [(lo, min(b, lo + per), CorrBlock(fmap1[lo:lo + per], fmap2[lo:lo + per], num_levels, radius, pyramid_dtype))
                            for lo in range(0, b, per)]
        else:
            self._build_or_record(fmap1, fmap2)

    def build(self, fmap1, fmap2):
        self.pyr: ops.TiledPyramid = ops.corr_build(fmap1, fmap2, self.half)

    @property
    def corr_pyramid(self):
        """The reference's attribute: [(B*Q, h_l, w_l) fp32 planes] (converted from the tiled storage on demand)."""
        if self._chunks is not None:
            return [torch.cat([blk.pyr.rowmajor(l) for _, _, blk in self._chunks], 0) for l in range(self.num_levels)]
        return [self.pyr.rowmajor(l) for l in range(self.num_levels)]

    def lookup(self, coords, out=None, want_taps=False):
        if self._chunks is None:
            return ops.corr_lookup_tiled(self.pyr, coords, want_taps, out=out)
        assert not want_taps, "taps of a chunked CorrBlock: ask the chunks"
        if out is None:
            b, h, w, _ = coords.shape
            out = ops.empty_nhwc(b, h, w, self._nk, coords)
        for lo, hi, blk in self._chunks:
            blk.lookup(coords[lo:hi], out=out[lo:hi])
        return out

    def grad_add(self, coords, dout):
        """Queued for grad_finish's one launch over the pass where that launch takes it (a query's four planes fit its
        LDS, at most ops.LOOKUP_BWD_ALL_MAX lookups); otherwise scattered into the zeroed gradient pyramid right away, the
        queue with it - large crops would keep every dout alive on top of that pyramid."""
        if (_LOOKUP_BWD_ALL and self.grad_pyr is None and len(self.pending) < ops.LOOKUP_BWD_ALL_MAX
                and ops.lookup_bwd_all_fits(self.pyr.h0, self.pyr.w0)):
            self.pending.append((coords, dout))
        else:
            pending, self.pending = self.pending, []
            self._scatter(pending + [(coords, dout)])

    def _scatter(self, pairs):
        if pairs and self.grad_pyr is None:
            p = self.pyr
            self.grad_pyr = ops.TiledPyramid.empty(p.levels[0].shape[0], p.h0, p.w0, False, p.levels[0].device, zero=True)
        for c, d in pairs:
            ops.corr_lookup_tiled_bwd(self.grad_pyr, c, d)

    def grad_finish(self, fmap1, fmap2):
        b, h, w, _ = fmap1.shape
        pending, self.pending = self.pending, []
        # the queue in one launch that folds the pooling chain too; a refusal here is a library change (grad_add checked the
        # plane sizes and the count): then launch by launch
        d0 = ops.corr_lookup_tiled_bwd_all([c for c, _ in pending], [d for _, d in pending], self.pyr.h0, self.pyr.w0) if pending else None
        if d0 is None:
            self._scatter(pending)
            gp, self.grad_pyr = self.grad_pyr, None
            if gp is None:
                return torch.zeros_like(fmap1), torch.zeros_like(fmap2)
            ops.corr_pyramid_tiled_bwd(gp)
            d0 = gp.levels[0]
        return ops.corr_volume_bwd(d0.view(b, h * w, -1), fmap1, fmap2, tiled=True)


class AlternateCorrBlock(_Block):
    """The reference's AlternateCorrBlock (FF_RAFT_Core/corr.py:63-91): CorrBlock's numbers (up to the order of the
    dot-product sums; the taps are bit-identical) without the all-pairs pyramid - memory linear in the image area, so a
    1088x1920 pair runs in fp32 and 2160x3840 at all.  NHWC fmaps (B, H8, W8, 256) fp32.

    ``build`` pools fmap2 once (ops.corr_alt_prepare); every lookup computes, per tile of queries, the dot products of the
    union of their windows on the matrix pipe and blends them (ops.corr_alt_lookup).  The backward of all of a pass's lookups
    runs at once in grad_finish (ops.corr_alt_lookup_bwd: one launch per 32 lookups, exact fp32 in every precision).
    ``corr_pyramid_dtype`` does not apply (nothing is stored per pair of positions); the lookup's arithmetic follows
    FF_CONV_PRECISION: three-term split f16 products, or exact fp32 ones under "fp32"."""
    pyr = None

    def __init__(self, fmap1: torch.Tensor, fmap2: torch.Tensor, num_levels: int = 4, radius: int = 4):
        super().__init__(num_levels, radius)
        self._build_or_record(fmap1, fmap2)

    def build(self, fmap1, fmap2):
        self._ops = ops.corr_alt_prepare(fmap1, fmap2)

    def lookup(self, coords, out=None, want_taps=False):
        return ops.corr_alt_lookup(self._ops, coords, want_taps, out=out)

    def grad_add(self, coords, dout):
        self.pending.append((coords, dout))

    def grad_finish(self, fmap1, fmap2):
        # (the launch reads the feature maps through the operands built from them)
        pending, self.pending = self.pending, []
        return ops.corr_alt_lookup_bwd(self._ops, [c for c, _ in pending], [d for _, d in pending])
