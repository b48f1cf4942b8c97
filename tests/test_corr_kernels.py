"""The materialised correlation block, kernel by kernel, against the fp64 references of tests/corr_ref.py.

Forward: ops.corr_lookup_tiled(..., want_taps=False) - the PRODUCT instance lookup_dma_kernel<HALF, false> that inference and
training launch (every other value test of the suite runs the debug instance) - at fractional coordinates, through deep
software pipelines (1 .. 6 queries per wave: planes 16x24 with up to 20 481 queries; the launch is 256 x 16 = 4 096 waves
and wave i takes queries i, i + 4096, ...), on the 1080p tile grid, into views of wider buffers.  Per output
    |out - out64| <= 8 x 2^-24 x absout64 + 1e-37
(four terms of at most four roundings each - 1 - wx, 1 - wy, the weight product, the value product - plus three additions;
absout64 is the blend of |values|), and the result equals the debug instance's bit for bit.

Gradient side, each kernel alone: ff_corr_lookup_tiled_bwd (grid-stride trips of its 5 120 blocks, accumulation into what is
there, views), ff_corr_pyramid_tiled_bwd (bit-equal to a float32 replay), ff_corr_lookup_tiled_bwd_all (its 16 384-block
grid-stride trip, integer coordinates = the mix of separable and LDS-atomic levels inside one query, the largest planes
that fit its LDS), ff_corr_tile_rows, ops.corr_volume_bwd.  Per element of a scattered plane
    |got - ref| <= (n + 8) x 2^-24 x S + 1e-37
with n the number of addends the element receives and S the same scatter of |dout| - both pooled down the chain where
the kernel pools (S with the chain's 0.25; n with 1: a parent's addends all arrive, and a count scaled by 0.25 would not
bound a sum in any order) - and every pad element of a tiled gradient plane is +0.0 bit for bit (csrc/corr_layout.h).
The contraction: (K + 4) x 2^-24 x abs-product / sqrt(C) + 1e-37, K the padded contraction length.

CorrBlock's gradient as a whole (section "bound of its own"): per tensor max|hip - ref64| <= 4 x max|ref32 - ref64| +
1e-6 x max|ref64|, ref32 the same six-channel reference in float32 on the CPU (the 4: another summation order over Q).

The CPU tests (no mark) check the references against the oracle's two lookups, scatter against lookup by adjointness, the
pool chain against autograd, that each listed mutation of a reference violates its bound by >= 10x on the inputs of the
GPU tests, and the conditions the cases are chosen for.

Out of scope: NaN coordinates, coordinates at or beyond 2^31 after scaling, pyramids near the lookup's 4 GB resource
limit, the lab-only variants FF_LOOKUP_DEPTH / FF_LOOKUP_BLOCK_WAVES.  Nothing here asks a kernel to fault.

Measured on an MI355X (largest error as a fraction of its bound, per group):
  * forward, product instance (bit-equal to the debug instance everywhere): pipeline depth 0.18 - 0.51 (Q = 1: 0.20 / 0.18
    fp32 / fp16; 4097: 0.45 / 0.48; 8191: 0.50 / 0.48; 12597: 0.45 / 0.49; 20481: 0.51 / 0.51); geometry 17x19 0.45 / 0.39,
    46x62 0.43 / 0.47, 68x120 0.53 / 0.52, 136x240 0.42 / 0.45.  The worst cases sit at half the bound because the bound
    counts the longest path's roundings at half an ulp each (seven of them, budget eight): the largest of the 2.6 million
    outputs of a case is a tail in which four of them line up; at integer coordinates, where the weights are 0 and 1, the
    result is exact.
  * ff_corr_lookup_tiled_bwd (zeroed, prefilled, twice; contiguous and view): 0.17 - 0.20 at Q = 1, 0.27 - 0.30 at Q = 300,
    0.34 / 0.33 at Q = 5121 / 10243; every pad +0.0.
  * ff_corr_pyramid_tiled_bwd: bit-equal to the float32 replay.
  * ff_corr_lookup_tiled_bwd_all: 16x24 T 1 Q 16400 0.21, 17x19 T 5 0.21, 23x31 T 12 0.22, 46x62 T 3 0.28, 48x64 T 2 0.28,
    16x24 T 32 0.10, 96x128 T 4 0.22.
  * ff_corr_tile_rows: exact.  ops.corr_volume_bwd: 0.005 - 0.014.
  * CorrBlock's gradient, max|hip - ref64| / max|ref32 - ref64| (largest per shape over recipes, pyramid dtypes and both
    scatter routes, where the error passes 1e-6 of max): 17x19 b 1: never passes it; b 3: 1.04 (T 1), 1.06 (T 3);
    46x62 b 1: 1.66 (T 1), 2.32 (T 3); b 3: 2.12 (T 1), 1.79 (T 3) - the largest ones on `discontinuous`, d fmap1.
"""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import corr_ref as R
from oracle import ffraft_ref as orc
from test_alt_corr import _coord_cases, alt_lookup_ref, _pooled
from test_alt_corr_backward import CHANS, _hip_grads, _ref_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = R.U
WILD = (1e6, -1e6, 3e7)                      # < 2^31 at every level
LOOKUP_WAVES = 4096                          # csrc/corr_lookup_dma.hip: 256 CUs x 16 waves, never more than the queries
BWD_BLOCKS, BWD_ALL_BLOCKS = 5120, 16384     # csrc/corr_lookup_tiled.hip: 256 x 20 and 256 x 64 blocks at most
PIPELINE_Q = (1, 4097, 8191, 12597, 20481)
GEOMETRY = [(17, 19, 323), (46, 62, 2852), (68, 120, 8160), (136, 240, 256)]
BWD_ALL_CASES = [(16, 24, 1, 16400), (17, 19, 5, 323), (23, 31, 12, 713), (46, 62, 3, 2852), (48, 64, 2, 3072),
                 (16, 24, 32, 64), (96, 128, 4, 40)]
BWD_CASES = [(17, 19, 1), (17, 19, 300), (17, 19, 5121), (17, 19, 10243), (20, 16, 1), (20, 16, 300), (23, 31, 1),
             (23, 31, 300), (46, 62, 1), (46, 62, 300)]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def positions(h, w, q):
    """Which grid position each of q queries stands for: the plane's own grid when q = h * w, a 16 x 16 grid over the plane
    for q = 256 on a larger plane, otherwise strided / cyclic."""
    n = h * w
    if q == n:
        return torch.arange(n)
    if q == 256 and n > 256:
        ys = torch.linspace(0, h - 1, 16).round().long()
        xs = torch.linspace(0, w - 1, 16).round().long()
        return (ys[:, None] * w + xs[None, :]).reshape(-1)
    return (torch.arange(q) * max(1, n // q)) % n


def border_coords(h, w):
    """The border set crossed in x and y: (121, 2)."""
    s = lambda n: torch.tensor([-5, -4.5, -4, -1, 0, n - 1, n, n + 3, n + 3.5, n + 4, n + 5], dtype=torch.float32)   # noqa: E731
    xs, ys = torch.meshgrid(s(w), s(h), indexing="ij")
    return torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)


def integer_coords(h, w, q):
    p = positions(h, w, q)
    return torch.stack([p % w, p // w], 1).float()


def mixed_coords(h, w, q, g, period=64, wild=False):
    """Uniform over [-12, w + 12] x [-12, h + 12] per query; every `period`-th query from the border set (neighbouring
    queries of a wave get unrelated windows); wild=True plants a wild value in x, y or both half a period later."""
    c = torch.rand(q, 2, generator=g) * torch.tensor([w + 24.0, h + 24.0]) - 12
    bc = border_coords(h, w)
    i = torch.arange(0, q, period)
    c[i] = bc[(i // period) % len(bc)]
    if wild:
        for n, j in enumerate(range(period // 2, q, period)):
            wx, wy = WILD[n % 3], WILD[(n // 3) % 3]
            c[j] = torch.tensor([(wx, wy), (wx, float(c[j, 1])), (float(c[j, 0]), wy)][(n // 9) % 3])
    return c


def recipes(h, w, q, g):
    """name -> (q, 2) float32 [x, y]: the nine cases of test_alt_corr (`integer` among them) on the positions the queries
    stand for, exact integers +- 2^-20, the crossed border set, wild values."""
    p = positions(h, w, q)
    out = {k: c[0].permute(1, 2, 0).reshape(h * w, 2)[p].contiguous() for k, c in _coord_cases(1, h, w, g).items()}
    base = out["integer"]
    sign = ((torch.arange(q) % 2) * 2 - 1).float().view(q, 1)
    out["integer_pm"] = base + sign * 2.0 ** -20
    bc = border_coords(h, w)
    out["border"] = bc[torch.arange(q) % len(bc)].clone()
    out["wild"] = mixed_coords(h, w, q, g, period=6, wild=True)
    return out


def waves_counts(q):
    """Queries per wave of the forward launch: min(q, 4096) waves, wave i takes q // waves (+ 1 if i < q % waves)."""
    nw = min(q, LOOKUP_WAVES)
    return {q // nw + (1 if i < q % nw else 0) for i in (0, nw - 1)}


def irregular_levels(coords, h, w):
    """(q, 4) bool x 2: level l of the query has non-consecutive taps (in x or y) / has a tap inside the plane."""
    irr, inside = [], []
    for l, (x0, y0, _, _) in enumerate(R.taps(coords, h, w)):
        hl, wl = h >> l, w >> l
        irr.append(((x0[:, 1:] - x0[:, :-1]) != 1).any(1) | ((y0[:, 1:] - y0[:, :-1]) != 1).any(1))
        xin = ((x0 >= 0) & (x0 < wl)) | ((x0 + 1 >= 0) & (x0 + 1 < wl))
        yin = ((y0 >= 0) & (y0 < hl)) | ((y0 + 1 >= 0) & (y0 + 1 < hl))
        inside.append(xin.any(1) & yin.any(1))
    return torch.stack(irr, 1), torch.stack(inside, 1)


@functools.lru_cache(maxsize=1)
def _planes(h, w, q):
    """Four (q, h_l, w_l) fp32 planes, N(0, 30^2) (independent levels: every kernel here treats them so)."""
    g = _gen(h, w, q, 1)
    return [torch.randn(q, h >> l, w >> l, generator=g) * 30 for l in range(4)]


def _bwd_all_inputs(h, w, T, q):
    g = _gen(h, w, T, q)
    cl = [integer_coords(h, w, q)] + [mixed_coords(h, w, q, g, period=16, wild=True) for _ in range(T - 1)]
    dl = [torch.randn(q, 324, generator=g) for _ in range(T)]
    return cl, dl


def _pooled_scatter(cl, dl, h, w, guard=True):
    """scatter_ref + pool_bwd_ref: level-0 (values, abs, counts) of what ff_corr_lookup_tiled_bwd_all computes."""
    v, s, n = R.scatter_ref(cl, dl, h, w)
    return (R.pool_bwd_ref(*v, guard=guard)[0], R.pool_bwd_ref(*s, guard=guard)[0], R.pool_bwd_ref(*n, scale=1.0, guard=guard)[0])


def _violation(mut, ref, bound):
    return ((mut - ref).abs() / bound).max().item()


def _report(group, frac):
    print(f"\ncorr_kernels {group}: {frac:.3f} of the bound")


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the references, the discrimination of the bounds, the case conditions
# ---------------------------------------------------------------------------------------------------------------------
def _nchw(c, h, w):
    return c.t().reshape(1, 2, h, w).contiguous()


@pytest.mark.parametrize("h,w", [(17, 19), (46, 62)])
def test_lookup_ref_against_the_oracles_two_lookups(h, w):
    """oracle.corr_lookup_explicit on double planes: the same taps, but its weights (1 - wx, 1 - wy and their product) are
    formed in fp32 - three roundings per term, so the two agree to 3 x 2^-24 x absout64 (+ 1e-12 of max for its fp64 sums),
    not to 1e-12 throughout; the from-scratch fp64 evaluation of the next test agrees to 1e-12.  oracle.corr_lookup in fp64
    (grid_sample) floors its own fp64 coordinate, so it is compared where every tap is >= 1e-3 away from an integer; its
    weights differ from the fp32 chain's by that chain's rounding: eight operations on |u| <= 128 move a tap by
    8 x 2^-24 x 128 = 6e-5 px, times the steepest slope 2 max|P| of a bilinear patch: 1.3e-4 of max."""
    q = h * w
    lv = [p.double() for p in _planes(h, w, q)]
    pyr = [p[:, None] for p in lv]
    for name, c in recipes(h, w, q, _gen(h, w, 2)).items():
        ref, aref = R.lookup_ref(lv, c)
        m = ref.abs().max().item()
        ex = orc.corr_lookup_explicit(pyr, _nchw(c, h, w))[0].permute(1, 2, 0).reshape(q, 324)
        assert ex.dtype == torch.float64
        assert ((ex - ref).abs() <= 3 * U * aref + 1e-12 * m).all(), name
        far = (c.abs() < 1e5).all(1)
        for x0, y0, wx, wy in R.taps(c, h, w):
            for f in (wx, wy):
                far &= ((f > 1e-3) & (f < 1 - 1e-3)).all(1)
        if far.any():
            gs = orc.corr_lookup(pyr, _nchw(c.double(), h, w))[0].permute(1, 2, 0).reshape(q, 324)
            assert (gs[far] - ref[far]).abs().max().item() <= 1.3e-4 * m, name


def test_lookup_ref_equals_a_from_scratch_evaluation_in_double():
    """lookup_ref against an fp64 evaluation of corr_lookup_explicit's formula on the same fp32 taps, written the other way
    round (explicit zero padding instead of masks): 1e-12 of max."""
    h, w = 17, 19
    q = h * w
    lv = [p.double() for p in _planes(h, w, q)]
    for name, c in recipes(h, w, q, _gen(h, w, 3)).items():
        ref, aref = R.lookup_ref(lv, c)
        outs = []
        for plane, (x0, y0, wx, wy) in zip(lv, R.taps(c, h, w)):
            hl, wl = plane.shape[-2:]
            pad = F.pad(plane, (12, 12, 12, 12))
            acc = torch.zeros(q, 9, 9, dtype=torch.float64)
            for dy in (0, 1):
                for dx in (0, 1):
                    xi = (x0 + dx).long().clamp(-12, wl + 11)[:, :, None].expand(q, 9, 9) + 12
                    yi = (y0 + dy).long().clamp(-12, hl + 11)[:, None, :].expand(q, 9, 9) + 12
                    v = pad[torch.arange(q).view(q, 1, 1), yi, xi]
                    acc += v * (wx.double() if dx else 1 - wx.double())[:, :, None] * (wy.double() if dy else 1 - wy.double())[:, None, :]
            outs.append(acc.view(q, 81))
        want = torch.cat(outs, 1)
        assert (want - ref).abs().max().item() <= 1e-12 * ref.abs().max().item(), name
        assert (aref >= ref.abs() - 1e-12 * aref.abs().max()).all()


@pytest.mark.parametrize("h,w,q", [(17, 19, 323), (16, 24, 500), (46, 62, 300)])
def test_scatter_ref_is_the_adjoint_of_lookup_ref(h, w, q):
    """<lookup_ref(P), D> == <P, scatter_ref(D)> for random P, D and every recipe: the scatter without autograd."""
    g = _gen(h, w, q, 4)
    lv = [torch.randn(q, h >> l, w >> l, generator=g, dtype=torch.float64) for l in range(4)]
    rec = recipes(h, w, q, g)
    rec["pipeline"] = mixed_coords(h, w, q, g)
    for name, c in rec.items():
        d = torch.randn(q, 324, generator=g)
        lhs = (R.lookup_ref(lv, c)[0] * d.double()).sum().item()
        planes, sabs, cnt = R.scatter_ref([c], [d], h, w)
        rhs = sum((p * x).sum().item() for p, x in zip(lv, planes))
        scale = sum((p.abs() * x).sum().item() for p, x in zip(lv, sabs))
        assert abs(lhs - rhs) <= 1e-12 * scale, (name, lhs, rhs)
        assert all((n >= 0).all() and n.max() <= 4 * 81 for n in cnt)


@pytest.mark.parametrize("h,w", [(17, 19), (23, 31), (46, 62), (16, 16)])
def test_pool_bwd_ref_against_autograd(h, w):
    g = _gen(h, w, 5)
    x = torch.randn(3, 1, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    lv = [x]
    for _ in range(3):
        lv.append(F.avg_pool2d(lv[-1], 2, stride=2))
    d = [torch.randn(3, h >> l, w >> l, generator=g, dtype=torch.float64) for l in range(4)]
    sum((a[:, 0] * b).sum() for a, b in zip(lv, d)).backward()
    got = R.pool_bwd_ref(*d)[0]
    assert (got - x.grad[:, 0]).abs().max().item() <= 1e-14 * got.abs().max().item()


def test_tiled_index_is_a_bijection_onto_the_non_pad_elements():
    for h0, w0 in [(17, 19), (46, 62), (16, 24), (136, 240)]:
        for half in (False, True):
            for l in range(4):
                off, pad = R.tiled_index(h0, w0, l, half)
                assert off.unique().numel() == off.numel() == (~pad).sum().item() and off.max().item() < pad.numel()
                he, we = R.tile_extent(h0, w0, l, half)
                assert he * we == pad.numel() and he >= h0 >> l and we >= w0 >> l


@pytest.mark.parametrize("mutation", ["shift_col", "swap_xy", "drop_last_row", "drop_last_col"])
def test_forward_bound_discriminates(mutation):
    """Each mutation of lookup_ref misses the forward bound by >= 10x on the geometry inputs (17 x 19: every recipe)."""
    h, w, q = 17, 19, 323
    lv = [p.double() for p in _planes(h, w, q)]
    worst = {}
    for name, c in recipes(h, w, q, _gen(h, w, q, 0)).items():
        ref, aref = R.lookup_ref(lv, c)
        worst[name] = _violation(R.lookup_ref(lv, c, mutate=mutation)[0], ref, 8 * U * aref + 1e-37)
    assert max(worst.values()) >= 10, worst
    # and on the pipeline inputs (16 x 24, every 64th query on the border set)
    h, w, q = 16, 24, 4097
    lv = [p.double() for p in _planes(h, w, q)]
    c = mixed_coords(h, w, q, _gen(q, 0))
    ref, aref = R.lookup_ref(lv, c)
    assert _violation(R.lookup_ref(lv, c, mutate=mutation)[0], ref, 8 * U * aref + 1e-37) >= 10


def test_scatter_bounds_discriminate():
    """A skipped lookup, an image that is not re-zeroed between two queries of a block, an ignored pad mask and a pool chain
    without its parent guard: each misses its bound by >= 10x on the inputs of the GPU tests."""
    # per-iteration scatter, 17 x 19, Q = 10 243: queries 5120.. are second, 10240.. third trips of their blocks (at
    # Q = 5121 only block 0 takes a second trip, and recipes that put query 0 far outside scatter nothing there)
    h, w, q = 17, 19, 2 * BWD_BLOCKS + 3
    second_trip_of_block_0 = {}
    for name, c in recipes(h, w, q, _gen(h, w, q, 6)).items():
        d = torch.randn(q, 324, generator=_gen(q, 7))
        v, s, n = R.scatter_ref([c], [d], h, w)
        for nq in (q, BWD_BLOCKS + 1):
            hit = 0.0
            for l in range(4):
                bound = ((n[l] + 8) * U * s[l] + 1e-37)[:nq]
                stale = v[l][:nq].clone()
                stale[BWD_BLOCKS:] += v[l][:nq - BWD_BLOCKS]
                hit = max(hit, _violation(stale, v[l][:nq], bound))
            if nq == q:
                assert hit >= 10, (name, hit)
            else:
                second_trip_of_block_0[name] = hit
        # pad mask ignored: elements of the tile grid beyond the plane receive something
        ext = [R.tile_extent(h, w, l) for l in range(4)]
        vp = R.scatter_ref([c[:400]], [d[:400]], h, w, extent=ext)[0]
        spill = sum(p[:, hl:, :].abs().sum().item() + p[:, :, wl:].abs().sum().item() for p, (hl, wl) in zip(vp, R.level_sizes(h, w)))
        if name in ("random", "border", "edge", "one_query", "integer"):
            assert spill > 0, name
    assert sum(v >= 10 for v in second_trip_of_block_0.values()) >= 8, second_trip_of_block_0      # (query 0 scatters nothing in some recipes)
    # one-launch scatter: a lookup skipped, the stale image at Q = 16 400 (16 384 blocks), the parent guard on odd planes
    for (h, w, T, q) in BWD_ALL_CASES:
        if q * h * w > 2 * 10 ** 6 and (T, q) != (1, 16400):
            continue                                                  # (the CPU suite stays quick: the small cases and the trip case)
        cl, dl = _bwd_all_inputs(h, w, T, q)
        v, s, n = _pooled_scatter(cl, dl, h, w)
        bound = (n + 8) * U * s + 1e-37
        if T > 1:
            assert _violation(_pooled_scatter(cl[:-1], dl[:-1], h, w)[0], v, bound) >= 10, (h, w, T, q)
            assert _violation(_pooled_scatter(cl[1:], dl[1:], h, w)[0], v, bound) >= 10, (h, w, T, q)
        if q > BWD_ALL_BLOCKS:
            stale = v.clone()
            stale[BWD_ALL_BLOCKS:] += v[:q - BWD_ALL_BLOCKS]
            assert _violation(stale, v, bound) >= 10
        if any((h >> l) % 2 or (w >> l) % 2 for l in range(3)):
            assert _violation(_pooled_scatter(cl, dl, h, w, guard=False)[0], v, bound) >= 10, (h, w, T, q)


@pytest.mark.parametrize("h,w", [(17, 19), (23, 31)])
def test_pool_replay_discriminates(h, w):
    """The float32 replay of the pool chain differs from an unguarded one on odd planes (bit equality is the bound)."""
    g = _gen(h, w, 8)
    d = [torch.randn(7, h >> l, w >> l, generator=g) for l in range(4)]
    assert not torch.equal(R.pool_bwd_ref(*d)[0], R.pool_bwd_ref(*d, guard=False)[0])


def test_case_conditions():
    """What the cases are chosen for, asserted: pipeline depths 1, 2, 3, 4 and >= 5; integer coordinates give queries whose
    levels mix the separable and the irregular path; the grid-stride cases pass their grids."""
    # the forward launch: waves = min(256 * wpc, queries) with wpc = max_wpc = 16, wave i takes queries i, i + waves, ...
    src = open(os.path.join(ROOT, "focusflow_official_amd", "csrc", "corr_lookup_dma.hip")).read()
    assert "256ll * wpc" in src and "max_wpc = deep ? 11 : 16" in src
    depths = set().union(*[waves_counts(q) for q in PIPELINE_Q])
    assert {1, 2, 3, 4} <= depths and max(depths) >= 5, depths
    assert waves_counts(4097) == {1, 2} and 4096 % LOOKUP_WAVES == 0        # query 4096 is the last query of wave 0 alone
    src = open(os.path.join(ROOT, "focusflow_official_amd", "csrc", "corr_lookup_tiled.hip")).read()
    assert ': 20;' in src and "256ll * bwd_wpc" in src and "256ll * 64" in src
    assert max(q for _, _, q in BWD_CASES) > 2 * BWD_BLOCKS and max(q for *_, q in BWD_ALL_CASES) > BWD_ALL_BLOCKS
    for (h, w, T, q) in BWD_ALL_CASES:
        irr, inside = irregular_levels(integer_coords(h, w, q), h, w)
        mixed = ((irr & inside).any(1) & (~irr).any(1)).sum().item()
        assert mixed >= 1, (h, w, q)
        assert sum((h >> l) * (w >> l) for l in range(4)) * 4 <= 64 * 1024
    # the counts the choice of planes rests on (queries with an irregular level that has taps inside the plane, per level)
    for (h, w), want in {(16, 24): [344, 214, 168, 0], (48, 64): [2154, 1274, 776, 636]}.items():
        irr, inside = irregular_levels(integer_coords(h, w, h * w), h, w)
        assert (irr & inside).sum(0).tolist() == want, (h, w, (irr & inside).sum(0).tolist())
        irr, inside = irregular_levels(integer_coords(h, w, h * w) + 0.5, h, w)
        assert (irr & inside).sum().item() == 0
    assert sum((96 >> l) * (128 >> l) for l in range(4)) * 4 == 65280


# ---------------------------------------------------------------------------------------------------------------------
# GPU: forward lookup, product instance
# ---------------------------------------------------------------------------------------------------------------------
def _pyramid(h, w, q, half):
    from focusflow_official_amd import ops
    pyr = ops.TiledPyramid.from_rowmajor([p.to(DEV) for p in _planes(h, w, q)], half)
    # fp16 storage: the reference sees the stored values
    lv64 = [pyr.rowmajor(l).cpu().double() for l in range(4)] if half else [p.double() for p in _planes(h, w, q)]
    return pyr, lv64


def _bits(t):
    return t.contiguous().view(torch.int32)


def _forward(pyr, lv64, c, what):
    """Product instance against fp64 and against the debug instance; returns the largest error / bound."""
    from focusflow_official_amd import ops
    q = c.shape[0]
    cd = c.view(1, 1, q, 2).contiguous().to(DEV)
    out = ops.corr_lookup_tiled(pyr, cd, want_taps=False)
    dbg, _ = ops.corr_lookup_tiled(pyr, cd, want_taps=True)
    torch.cuda.synchronize()
    ndiff = (_bits(out) != _bits(dbg)).sum().item()
    assert ndiff == 0, f"{what}: product and debug instance differ in {ndiff} outputs"
    ref, aref = R.lookup_ref(lv64, c)
    frac = ((out.cpu().view(q, 324).double() - ref).abs() / (8 * U * aref + 1e-37)).max().item()
    assert frac <= 1, f"{what}: |out - fp64| is {frac:.2f} x the bound"
    return frac


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("q", PIPELINE_Q)
def test_forward_pipeline_depth(q, half):
    h, w = 16, 24
    pyr, lv64 = _pyramid(h, w, q, half)
    frac = _forward(pyr, lv64, mixed_coords(h, w, q, _gen(q, 0)), f"pipeline Q={q}")
    _report(f"forward pipeline Q={q} {'fp16' if half else 'fp32'} (queries per wave {sorted(waves_counts(q))})", frac)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("h,w,q", GEOMETRY)
def test_forward_geometry(h, w, q, half):
    pyr, lv64 = _pyramid(h, w, q, half)
    fr = {name: _forward(pyr, lv64, c, f"{h}x{w} {name}") for name, c in recipes(h, w, q, _gen(h, w, q, 0)).items()}
    worst = max(fr, key=fr.get)
    _report(f"forward geometry {h}x{w} Q={q} {'fp16' if half else 'fp32'} (worst: {worst})", fr[worst])


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_forward_output_views(half):
    """Into out=buf[..., :324] of a 352-wide buffer, as inference does: channels 324..351 keep their bits; and the last-query
    case (Q = 4097: wave 0 alone has a second query) inside a buffer one row longer: the row after the last keeps its bits."""
    from focusflow_official_amd import ops
    h, w, q = 16, 24, 4097
    pyr, _ = _pyramid(h, w, q, half)
    cd = mixed_coords(h, w, q, _gen(q, 0)).view(1, 1, q, 2).to(DEV)
    want = ops.corr_lookup_tiled(pyr, cd)
    pattern = torch.tensor(0x7fc0beef, dtype=torch.int32)          # a quiet NaN with a payload
    for ld in (352, 324):
        buf = torch.full((1, 1, q + 1, ld), 0, dtype=torch.int32, device=DEV).fill_(pattern.item()).view(torch.float32)
        ops.corr_lookup_tiled(pyr, cd, out=buf[:, :, :q, :324])
        torch.cuda.synchronize()
        b = _bits(buf)
        assert torch.equal(_bits(buf[:, :, :q, :324]), _bits(want)), ld
        assert (b[:, :, :q, 324:] == pattern.item()).all() and (b[:, :, q] == pattern.item()).all(), ld


# ---------------------------------------------------------------------------------------------------------------------
# GPU: gradient kernels, each alone
# ---------------------------------------------------------------------------------------------------------------------
def _rowmajor(t, h0, w0, level):
    """(Q, plane) tiled fp32 on the GPU -> ((Q, h_l, w_l) fp64 there, pads all +0.0).  (The comparisons of the gradient
    planes run in fp64 on the GPU: the references come from the CPU, the large-Q cases would spend their time in host copies.)"""
    off, pad = R.tiled_index(h0, w0, level, False)
    assert t.shape[1] == pad.numel()
    return (t[:, off.reshape(-1).to(t.device)].double().view(t.shape[0], *off.shape),
            bool((_bits(t)[:, pad.to(t.device)] == 0).all().item()))


def _zero_pyr(q, h, w):
    from focusflow_official_amd import ops
    return ops.TiledPyramid.empty(q, h, w, False, torch.device(DEV), zero=True)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,q", BWD_CASES)
def test_lookup_tiled_bwd_against_fp64(h, w, q):
    """ff_corr_lookup_tiled_bwd: into zeroed planes, into prefilled planes (read-modify-write keeps what was there), two
    launches in succession; dout contiguous and as a view of a 352-wide buffer whose pad channels are NaN."""
    from focusflow_official_amd import ops
    g = _gen(h, w, q, 9)
    pre = [torch.randn(q, h >> l, w >> l, generator=g).to(DEV) for l in range(4)]
    worst = 0.0
    for name, c in recipes(h, w, q, g).items():
        d = torch.randn(q, 324, generator=g)
        v, s, n = ([p.to(DEV) for p in x] for x in R.scatter_ref([c], [d], h, w))
        cd = c.view(1, 1, q, 2).contiguous().to(DEV)
        wide = torch.full((1, 1, q, 352), float("nan"))
        wide[..., :324] = d
        wide = wide.to(DEV)
        for layout, dd in (("contiguous", d.view(1, 1, q, 324).to(DEV)), ("view", wide[..., :324])):
            runs = {"zeroed": (_zero_pyr(q, h, w), 1, None), "prefilled": (ops.TiledPyramid.from_rowmajor(pre), 1, pre),
                    "twice": (_zero_pyr(q, h, w), 2, None)}
            for run, (dp, times, fill) in runs.items():
                for _ in range(times):
                    ops.corr_lookup_tiled_bwd(dp, cd, dd)
                torch.cuda.synchronize()
                for l in range(4):
                    got, pads_zero = _rowmajor(dp.levels[l], h, w, l)
                    assert pads_zero, f"{name} {layout} {run}: level {l} has a pad element that is not +0.0"
                    ref, sc, cnt = v[l] * times, s[l] * times, n[l] * times + 8
                    if fill is not None:                      # one more addend, one more rounding
                        ref, sc, cnt = ref + fill[l].double(), sc + fill[l].double().abs(), cnt + 1
                    frac = ((got - ref).abs() / (cnt * U * sc + 1e-37)).max().item()
                    assert frac <= 1, f"{name} {layout} {run} level {l}: {frac:.2f} x the bound"
                    worst = max(worst, frac)
    _report(f"lookup_tiled_bwd {h}x{w} Q={q}", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("q", [1, 7])
@pytest.mark.parametrize("h,w", [(16, 16), (17, 19), (23, 31), (46, 62)])
def test_pyramid_tiled_bwd_is_the_float32_replay(h, w, q):
    """Levels 2, 1, 0 afterwards: v + 0.25f * parent, one rounding per element (0.25f * parent is exact), fixed order -
    bit equality; level 3 unchanged; pads zero."""
    from focusflow_official_amd import ops
    g = _gen(h, w, q, 10)
    d = [torch.randn(q, h >> l, w >> l, generator=g) for l in range(4)]
    dp = ops.TiledPyramid.from_rowmajor([p.to(DEV) for p in d])
    before3 = dp.levels[3].clone()
    ops.corr_pyramid_tiled_bwd(dp)
    torch.cuda.synchronize()
    want = R.pool_bwd_ref(*d)                               # float32 in, float32 arithmetic
    assert all(x.dtype == torch.float32 for x in want)
    assert torch.equal(_bits(dp.levels[3]), _bits(before3))
    for l in range(4):
        off, pad = R.tiled_index(h, w, l, False)
        t = dp.levels[l].cpu()
        assert (_bits(t)[:, pad] == 0).all(), f"level {l}: pad not +0.0"
        assert torch.equal(_bits(t[:, off.reshape(-1)]), _bits(want[l].reshape(q, -1))), f"level {l} is not the float32 replay"


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,T,q", BWD_ALL_CASES)
def test_lookup_tiled_bwd_all_against_fp64(h, w, T, q):
    """ff_corr_lookup_tiled_bwd_all against scatter_ref + pool_bwd_ref; lookup 0 at integer coordinates."""
    from focusflow_official_amd import ops
    cl, dl = _bwd_all_inputs(h, w, T, q)
    d0 = ops.corr_lookup_tiled_bwd_all([c.view(1, 1, q, 2).to(DEV) for c in cl], [d.view(1, 1, q, 324).to(DEV) for d in dl], h, w)
    assert d0 is not None
    torch.cuda.synchronize()
    got, pads_zero = _rowmajor(d0, h, w, 0)
    assert pads_zero, "d0 has a pad element that is not +0.0"
    v, s, n = (x.to(DEV) for x in _pooled_scatter(cl, dl, h, w))
    frac = ((got - v).abs() / ((n + 8) * U * s + 1e-37)).max().item()
    _report(f"lookup_tiled_bwd_all {h}x{w} T={T} Q={q}", frac)
    assert frac <= 1, f"{frac:.2f} x the bound"


@pytest.mark.gpu
def test_lookup_tiled_bwd_all_declines():
    from focusflow_official_amd import ops
    z = lambda q: torch.zeros(1, 1, q, 2, device=DEV)                  # noqa: E731
    d = lambda q: torch.zeros(1, 1, q, 324, device=DEV)                # noqa: E731
    assert ops.corr_lookup_tiled_bwd_all([z(4)] * 33, [d(4)] * 33, 16, 24) is None
    assert ops.corr_lookup_tiled_bwd_all([z(8)], [d(8)], 128, 160) is None
    assert ops.corr_lookup_tiled_bwd_all([z(4)] * 32, [d(4)] * 32, 16, 24) is not None


@pytest.mark.gpu
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("h,w", [(17, 19), (46, 62)])
def test_tile_rows(h, w, b):
    from focusflow_official_amd import ops
    x = torch.randn(b, h * w, 256, generator=_gen(h, w, b, 11))
    t = ops.corr_tile_rows(x.to(DEV), h, w, True)
    back = ops.corr_tile_rows(t, h, w, False)
    torch.cuda.synchronize()
    off, pad = R.tiled_index(h, w, 0, False)
    t = t.cpu()
    assert t.shape == (b, pad.numel(), 256)
    assert torch.equal(_bits(back.cpu()), _bits(x))
    assert torch.equal(_bits(t[:, off.reshape(-1)]), _bits(x))
    assert (_bits(t[:, pad]) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("tiled", [False, True], ids=["rowmajor", "tiled"])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("h,w", [(16, 24), (17, 19)])
def test_volume_bwd_against_fp64(h, w, b, tiled):
    from focusflow_official_amd import ops
    g = _gen(h, w, b, 12)
    q, c = h * w, 256
    f1, f2 = torch.randn(b, h, w, c, generator=g), torch.randn(b, h, w, c, generator=g)
    dvol = torch.randn(b, q, q, generator=g)
    off, pad = R.tiled_index(h, w, 0, False)
    if tiled:
        dv = torch.zeros(b, q, pad.numel())
        dv[:, :, off.reshape(-1)] = dvol
        k1 = pad.numel()
    else:
        dv, k1 = dvol, (q + 3) // 4 * 4
    df1, df2 = ops.corr_volume_bwd(dv.to(DEV), f1.to(DEV), f2.to(DEV), tiled=tiled)
    torch.cuda.synchronize()
    r1, r2, a1, a2 = R.volume_bwd_ref(dvol, f1.view(b, q, c), f2.view(b, q, c))
    s = c ** -0.5
    worst = 0.0
    for what, got, ref, ab, k in (("df1", df1, r1, a1, k1), ("df2", df2, r2, a2, (q + 3) // 4 * 4)):
        frac = ((got.cpu().view(b, q, c).double() - ref).abs() / ((k + 4) * U * ab * s + 1e-37)).max().item()
        assert frac <= 1, f"{what}: {frac:.2f} x the bound"
        worst = max(worst, frac)
    _report(f"volume_bwd {h}x{w} b={b} {'tiled' if tiled else 'rowmajor'}", worst)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: CorrBlock's gradient, a bound of its own
# ---------------------------------------------------------------------------------------------------------------------
def _ref_grads32(f1, f2, coords_list, douts, chans=CHANS):
    """test_alt_corr_backward._ref_grads, evaluated in float32."""
    a = f1[:, chans].clone().requires_grad_(True)
    b = f2[:, chans].clone().requires_grad_(True)
    lv = _pooled(b)
    loss = 0
    for c, d in zip(coords_list, douts):
        if d is not None:
            loss = loss + (alt_lookup_ref(a, lv, c) * d).sum()
    (loss * (len(chans) ** 0.5 / 16.0)).backward()
    return a.grad, b.grad


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("h,w", [(17, 19), (46, 62)])
def test_corr_block_gradient_against_fp64(h, w, b, T, monkeypatch):
    """Every recipe of test_alt_corr, fp32 and fp16 pyramids (the gradient is straight-through: the same), the one-launch
    scatter on and off."""
    from focusflow_official_amd import corr_block
    g = _gen(h, w, b, T, 13)
    f1, f2 = torch.randn(b, 256, h, w, generator=g), torch.randn(b, 256, h, w, generator=g)
    worst = (0.0, "")
    for name, c in _coord_cases(b, h, w, g).items():
        cl = [c + (torch.rand(c.shape, generator=g) - 0.5) * 2 * t for t in range(T)]
        douts = [torch.randn(b, 324, h, w, generator=g) for _ in range(T)]
        if T == 3:
            douts[1] = None
        r64, r32 = _ref_grads(f1, f2, cl, douts), _ref_grads32(f1, f2, cl, douts)
        for dtype in ("fp32", "fp16"):
            for one_launch in (True, False):
                monkeypatch.setattr(corr_block, "_LOOKUP_BWD_ALL", one_launch)
                got = _hip_grads(corr_block.CorrBlock, f1, f2, cl, douts, pyramid_dtype=dtype)
                for what, hip, a64, a32 in zip(("d fmap1", "d fmap2"), got, r64, r32):
                    e = (hip[:, CHANS].double() - a64).abs().max().item()
                    e32, m = (a32.double() - a64).abs().max().item(), a64.abs().max().item()
                    ratio = e / max(e32, 1e-300)
                    if e > 1e-6 * m and ratio > worst[0]:
                        worst = (ratio, f"{name} {dtype} one_launch={one_launch} {what}")
                    assert e <= 4 * e32 + 1e-6 * m, f"{name} T={T} {dtype} one_launch={one_launch} {what}: {e:.3e} vs ref32's {e32:.3e} (max {m:.3e})"
    print(f"\ncorr_kernels CorrBlock gradient {h}x{w} b={b} T={T}: max|hip - ref64| / max|ref32 - ref64| up to {worst[0]:.2f} ({worst[1]})")
