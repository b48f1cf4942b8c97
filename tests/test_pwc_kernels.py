"""Operator tests of FF-PWC's native kernels, each against a plain fp64 reference on the CPU (tests/pwc_kernel_ref.py:
oracle.pwc_ref in fp64, autograd for the gradients): the cost volume forward in both modes (costvolume_fwd_kernel<false|true>,
cv_finish_kernel), its backward (costvolume_bwd_kernel, gout_transpose_kernel) with the two autograd wrappers, backwarp forward
and backward, and the direct transposed convolution (deconv4x4s2_small_kernel).

Inputs are drawn in fp32 and the same fp32 values go to both sides.  A "view" is a channel slice of a wider buffer whose
surroundings hold SENTINEL: `one` / `two` / feature maps at channel 4 of a buffer 8 channels wider, the volume in channels
[448, 529) of a 704-wide level buffer, the deconvolution's output in the 16-wide slot at channel 564 of such a buffer,
backwarp's flow in channels [0, 2) of a 16-wide slot at channel 8 of a 32-wide buffer.  After every call the input buffers
are bit-identical to their snapshots and the surroundings of an output view still hold SENTINEL (the three pad channels of
an 84-wide gradient that is only read too).
A second call on the same inputs is bit-identical for every kernel but d_input of backwarp, which is accumulated with fp32
atomics in no fixed order and is held to the value check only.

Cases
  cost volume (B, C, H, W) and the splits pwc._cv_fwd asks for -> what the library makes of them:
      (1, 4, 1, 1) 1    (1, 20, 3, 5) 1    (2, 32, 17, 35) 1    (1, 196, 7, 16) 13 -> 13    (4, 96, 28, 64) 4 -> 3
      (1, 64, 60, 100) 4 -> 4    (1, 8, 100, 131) 1
    each with explicit splits {0, 2, 3, chunks, chunks + 5} (one chunk: 0 only), act NONE / LEAKY, contiguous and as views;
    the backward and gout_transpose with g_ld 81 and 84; FunctionCorrelation and _CostVolume84 with gradients for both
    inputs, `one` only, `two` only.
  backwarp (B, C, H, W, flow_scale, sd): (2, 32, 28, 40, 5.0, 1.5)  (1, 196, 7, 16, 0.625, 1.5)  (1, 64, 17, 23, 2.5, 1.5)
      (1, 4, 2, 2, 1.25, 0.3)  (3, 8, 5, 33, 1.25, 2.0)  (1, 128, 128, 260, 5.0, 4.0); sd of the last one is 4.0 because at 1.5
      93 % of its pixels are valid, at 4.0 81 % (a tenth of the plane has to show either outcome).  Edge inputs at 17 x 23:
      flow zero, whole-pixel shifts, the validity threshold on all four borders, flows far outside.
  deconvolution (Cin, Cout, B, H, W): (4, 1, 1, 1, 1)  (256, 2, 1, 3, 5)  (260, 2, 2, 3, 5)  (544, 2, 1, 7, 16)  (704, 2, 1, 5, 9),
      with and without bias, x full width and as a view, the output 16 wide on its own (ld 16) and as the 16-wide slot of a 704-wide buffer.

Value checks.  Cost volume and deconvolution: |got - fp64| <= (n + 3) * 2^-24 * sum|a_i b_i| per element
(pwc_kernel_ref.check_bound; n = C forward, 81 backward, 4 Cin + 1 deconvolution), exactly zero where that sum is zero.
Largest fraction of the bound reached (CPU fp32 oracle: 0.34 forward at C = 8, <= 0.07 elsewhere; MI355X: see below):

    kernel                                  largest fraction of the bound on the MI355X
    costvolume_fwd, unsplit                 0.264   (C = 8, 100 x 131: n + 3 = 11; every other case <= 0.10)
    costvolume_fwd, split + cv_finish       0.054
    costvolume_bwd (grad one and grad two)  0.071
    deconv4x4s2_small                       0.040

Backwarp has no such bound (its error is the rounding of the sample position times the local slope of the input, and it is
discontinuous at the validity threshold, d_flow at the cell borders too).  Pixels are left out from the fp64 reference alone:
weight sum within tau of 0.999 (everything), valid and within tau of a cell border (d_flow); tau = 4 x the largest fp32-fp64
difference of the reference's own sample position, at least 1e-5; the upstream gradient is zero at the pixels left out.
The tolerance is 4 x the error of the fp32 CPU oracle against the fp64 one on the pixels left, in the measure
max |a - ref| / (|ref| + max|ref|).  Per case: tau, share left out of d_flow (nothing is left out at the threshold), then
CPU fp32 error / MI355X error for out, d_input, d_flow (tolerance = 4 x the first number of each pair):

    case                          tau       left out   out                    d_input                d_flow
    (2, 32, 28, 40, 5.0, 1.5)     2.50e-05  4.46e-04   2.69e-06 / 3.09e-06    2.20e-06 / 2.71e-06    1.99e-06 / 2.02e-06
    (1, 196, 7, 16, 0.625, 1.5)   1.00e-05  0          7.06e-07 / 7.75e-07    4.50e-07 / 4.54e-07    3.36e-07 / 3.17e-07
    (1, 64, 17, 23, 2.5, 1.5)     1.00e-05  0          1.58e-06 / 1.58e-06    9.36e-07 / 1.03e-06    1.42e-06 / 1.47e-06
    (1, 4, 2, 2, 1.25, 0.3)       1.00e-05  0          1.97e-07 / 1.97e-07    7.03e-08 / 7.03e-08    3.24e-08 / 3.24e-08
    (3, 8, 5, 33, 1.25, 2.0)      1.24e-05  0          1.97e-06 / 1.97e-06    1.10e-06 / 1.11e-06    1.22e-06 / 1.23e-06
    (1, 128, 128, 260, 5.0, 4.0)  1.60e-04  7.21e-04   1.86e-05 / 1.99e-05    1.19e-05 / 1.19e-05    1.52e-05 / 1.54e-05

The kernel stays within 1.25 x the CPU's fp32 error everywhere: both carry the same dominant terms, the fp32 rounding of
flow * flow_scale and of the grid coordinate (position error up to 4.0e-05 pixels at W = 260).  The edge inputs (tolerances of
the 17 x 23 case: 6.3e-06 out, 3.7e-06 d_input) reach 1.81e-06 at most.  No kernel exceeded a bound or a tolerance; none changed.
"""
import pytest
import torch
import torch.nn.functional as F

import pwc_kernel_ref as R

gpu = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = R.SENTINEL
VOL_LEAD, FLOW_LEAD, LEVEL_WIDTH, SLOT = 448, 564, 704, 16        # pwcnet.Decoder.run: volume, flow slot, widest level buffer
FLOW_BUF = (8, 32)      # backwarp's flow: channels [0, 2) of the 16-wide slot at channel 8 of a 32-wide buffer (the big case stays small)


class _Lib:
    def __init__(self):
        from focusflow_official_amd import _hip, ops, pwc, pwcnet
        self.hip, self.ops, self.pwc, self.pwcnet = _hip, ops, pwc, pwcnet
        self.p, self.ld, self.stream = ops._p, ops._ld, ops._stream

    def call(self, name, *args):
        self.hip.call(name, *args)


@pytest.fixture(scope="module")
def lib():
    yield _Lib()
    print("\nlargest value per kernel:", {k: f"{v:.3e}" for k, v in sorted(R.MEASURED.items())})


def put(t, view, guards, lead=4, width=None):
    """CPU tensor -> device tensor; as a view it sits in channels [lead, lead + C) of a SENTINEL-filled buffer of `width`."""
    if not view:
        return t.to(DEV)
    c = t.shape[-1]
    buf = torch.full((*t.shape[:-1], width or c + 8), SENTINEL, dtype=t.dtype, device=DEV)
    buf[..., lead:lead + c] = t.to(DEV)
    guards.append((buf, buf.clone()))
    return buf[..., lead:lead + c]


def out_buf(shape, view, lead=4, width=None, fill=SENTINEL):
    """-> (buffer, the output tensor inside it): contiguous, or channels [lead, lead + C) of a SENTINEL buffer; the output
    itself starts as `fill`."""
    c = shape[-1]
    if not view:
        out = torch.full(shape, fill, dtype=torch.float32, device=DEV)
        return out, out
    buf = torch.full((*shape[:-1], width or c + 8), SENTINEL, dtype=torch.float32, device=DEV)
    buf[..., lead:lead + c] = fill
    return buf, buf[..., lead:lead + c]


def untouched(guards):
    return all(torch.equal(buf, snap) for buf, snap in guards)


def surroundings_kept(buf, out, lead):
    if buf is out:
        return True
    return bool((buf[..., :lead] == SENTINEL).all()) and bool((buf[..., lead + out.shape[-1]:] == SENTINEL).all())


# =====================================================================================================================
# CPU: the tables, the exclusion caps, the oracle's dtype
def test_case_tables_hold_what_they_are_for():
    for c in R.CV_CASES:
        assert R.cv_product_splits(c) == c.product_splits and R.cv_library_splits(c.C, c.product_splits) == c.library_splits, c
        assert c.C % 4 == 0
    by = {(c.B, c.C, c.H, c.W): c for c in R.CV_CASES}
    assert R.cv_channels_per_split(96, 4) == 32 and by[(4, 96, 28, 64)].library_splits == 3       # 2 chunks each, 3 splits
    assert 196 % 16 == 4 and by[(1, 196, 7, 16)].product_splits == 13
    assert 60 * 100 * 81 > 1024 * 256 and by[(1, 64, 60, 100)].product_splits > 1                   # cv_finish_kernel's cap
    assert 100 * 131 * 81 > 4096 * 256                                                              # gout_transpose_kernel's cap
    assert bool((R.cv_reference(by[(1, 4, 1, 1)])["abs_vol"] == 0).sum() == 80)
    assert R.cv_splits(by[(1, 4, 1, 1)]) == [0] and R.cv_splits(by[(4, 96, 28, 64)]) == [0, 2, 3, 6, 11]
    big = R.BW_CASES[-1]
    assert big.B * big.H * big.W > 8192 * 4 and big.B * big.H * big.W * (big.C // 4) > 4096 * 256   # both backwarp caps
    assert any(c.Cin == 256 for c in R.DC_CASES) and any(c.Cin == 260 for c in R.DC_CASES)


@pytest.mark.parametrize("case", R.BW_CASES, ids=R.bw_case_id)
def test_backwarp_cases_leave_out_little_and_show_both_outcomes(case):
    """No GPU: from the fp64 reference alone, at most a thousandth of the pixels is left out, and valid and invalid pixels
    each cover at least a tenth of the plane."""
    ref = R.bw_reference(case)
    ex = ref["ex"]
    share = float((ex["near_thr"] | ex["near_int"]).double().mean())
    valid = float(ex["valid"].double().mean())
    print(f"{R.bw_case_id(case)}: tau {ex['tau']:.2e} (position error {ex['pos_err']:.2e}), left out {share:.2e}, valid {valid:.3f}, "
          f"fp32 CPU error {ref['cpu_err']}")
    assert ex["tau"] >= R.TAU_FLOOR and ex["tau"] >= 4 * ex["pos_err"]
    assert share <= 1e-3
    assert 0.1 <= valid <= 0.9
    assert bool((ref["gout"][ex["near_thr"]] == 0).all())
    assert all(v > 0 for v in ref["cpu_err"].values())


def test_edge_inputs_are_what_they_claim():
    """No GPU: the edge inputs' fp64 sample positions - whole pixels, 0.0005 / 0.0015 outside the borders."""
    c = R.EDGE_CASE
    for dx, dy in R.SHIFTS:
        ex = R.bw_exclusions(R.flow_for_offset(float(dx), float(dy)), c.scale)
        xs, ys = torch.arange(c.W).view(1, 1, c.W).double(), torch.arange(c.H).view(1, c.H, 1).double()
        assert float((ex["ux"] - xs - dx).abs().max()) < 1e-6 and float((ex["uy"] - ys - dy).abs().max()) < 1e-6
    flow, valid_px, invalid_px = R.threshold_input()
    ws = R.bw_exclusions(flow, c.scale)["wsum"][0]
    assert int(valid_px.sum()) + int(invalid_px.sum()) == 2 * c.H + 2 * (c.W - 2) and int(valid_px.sum()) >= 30 and int(invalid_px.sum()) >= 30
    assert float((ws[valid_px] - 0.9995).abs().max()) < 1e-6 and float((ws[invalid_px] - 0.9985).abs().max()) < 1e-6
    assert bool((ws[~(valid_px | invalid_px)] == 1).all())
    for border in (valid_px, invalid_px):          # both outcomes on each of the four borders
        assert border[1:-1, 0].any() and border[1:-1, -1].any() and border[0, 1:-1].any() and border[-1, 1:-1].any()


# =====================================================================================================================
# CPU: the checks discriminate.  Each planted fault goes through the check function the GPU tests call.
def _cv196():
    case = next(c for c in R.CV_CASES if c.C == 196)
    return case, R.cv_reference(case)


def test_planted_cost_volume_faults_fail_the_check():
    from oracle import pwc_ref
    case, ref = _cv196()
    one, two = R.nchw(ref["one"]), R.nchw(ref["two"])
    good = R.nhwc(pwc_ref.cost_volume(one, two))
    assert R.check_bound("cpu fp32 oracle", good, ref["vol"], ref["abs_vol"], case.C, "fp32 oracle") < 0.09
    dropped = R.nhwc(pwc_ref.cost_volume(one[:, :192], two[:, :192]) * (192 / 196))
    with pytest.raises(AssertionError, match="of the derived bound"):
        R.check_bound("planted", dropped, ref["vol"], ref["abs_vol"], case.C, "channels 192 to 195 dropped")
    swapped = good.view(*good.shape[:3], 9, 9).transpose(3, 4).reshape(good.shape)
    with pytest.raises(AssertionError, match="x and y displacement swapped"):      # (either message: the padded channels move too)
        R.check_bound("planted", swapped, ref["vol"], ref["abs_vol"], case.C, "x and y displacement swapped")
    # (the restatement of the split mode itself passes, in both activations)
    for act in (R.ACT_NONE, R.ACT_LEAKY):
        want = ref["vol"] if act == R.ACT_NONE else F.leaky_relu(ref["vol"], 0.1)
        R.check_bound("cpu split restatement", R.cv_split_restatement(ref["one"], ref["two"], 3, act), want, ref["abs_vol"], case.C, f"3 splits act {act}")
    with pytest.raises(AssertionError, match="of the derived bound"):
        R.check_bound("planted", R.cv_split_restatement(ref["one"], ref["two"], 13, R.ACT_NONE, drop_last=True), ref["vol"], ref["abs_vol"],
                      case.C, "last split's partial left out")
    with pytest.raises(AssertionError, match="of the derived bound"):
        R.check_bound("planted", R.cv_split_restatement(ref["one"], ref["two"], 3, R.ACT_LEAKY, act_per_split=True),
                      F.leaky_relu(ref["vol"], 0.1), ref["abs_vol"], case.C, "leaky per split")
    # a padded displacement that is not exactly zero
    case1 = R.CV_CASES[0]
    r1 = R.cv_reference(case1)
    leak = r1["vol"].float().clone()
    leak[..., 0] = 1e-30
    with pytest.raises(AssertionError, match="padding"):
        R.check_bound("planted", leak, r1["vol"], r1["abs_vol"], case1.C, "value in a padded displacement")


def test_planted_backwarp_faults_fail_the_check():
    case = R.EDGE_CASE
    ref = R.bw_reference(case)
    x, flow = R.nchw(ref["x"]), R.nchw(ref["flow"]) * case.scale
    good = R.nhwc(R.backwarp_variant(x, flow))
    R.check_rel("cpu fp32 restatement", good, ref["out"], ref["tol"]["out"], "restatement", ref["keep"])
    with pytest.raises(AssertionError, match="needs a tolerance"):
        R.check_rel("planted", R.nhwc(R.backwarp_variant(x, flow, align_corners=True)), ref["out"], ref["tol"]["out"], "align_corners=True", ref["keep"])
    # the validity test written as > 0.99: pixels with weight sum 0.9985 come out non-zero
    xe, _ = R.edge_data()
    tflow, valid_px, invalid_px = R.threshold_input()
    want, _, _ = R.bw_oracle(xe, tflow, case.scale, torch.zeros_like(xe), torch.float64)
    ok = R.nhwc(R.backwarp_variant(R.nchw(xe), R.nchw(tflow) * case.scale))
    R.check_threshold_forward("cpu fp32 restatement", ok, want, valid_px, invalid_px, ref["tol"]["out"])
    loose = R.nhwc(R.backwarp_variant(R.nchw(xe), R.nchw(tflow) * case.scale, threshold=0.99))
    with pytest.raises(AssertionError, match="not exactly zero"):
        R.check_threshold_forward("planted", loose, want, valid_px, invalid_px, ref["tol"]["out"])


def test_planted_deconvolution_fault_fails_the_check():
    case = R.DC_CASES[2]
    ref = R.dc_reference(case)
    x = R.nchw(ref["x"])
    good = R.nhwc(F.conv_transpose2d(x, ref["wt"], ref["bias"], stride=2, padding=1))
    assert R.check_bound("cpu fp32 oracle", good, ref["ref"], ref["abs"], 4 * case.Cin + 1, "fp32 conv_transpose2d") < 0.09
    unflipped = R.nhwc(F.conv_transpose2d(x, ref["wt"].flip(2, 3), ref["bias"], stride=2, padding=1))
    with pytest.raises(AssertionError, match="of the derived bound"):
        R.check_bound("planted", unflipped, ref["ref"], ref["abs"], 4 * case.Cin + 1, "kernel not flipped")


def test_gout_transpose_restatement_is_the_adjoint_route():
    """No GPU: grad two = the grad-one formula applied to the transposed gradient (what the kernels rely on), in fp64."""
    from oracle import pwc_ref
    case = R.CV_CASES[1]
    ref = R.cv_reference(case)
    gt = R.nchw(R.gout_transpose_ref(ref["gy"])).double()
    one = R.nchw(ref["one"]).double()
    pad = F.pad(one, (4, 4, 4, 4))
    g_two = sum(gt[:, d:d + 1] * pad[:, :, d // 9:d // 9 + case.H, d % 9:d % 9 + case.W] for d in range(81)) / case.C
    assert torch.allclose(R.nhwc(g_two), ref["g_two"], rtol=1e-12, atol=1e-13)
    assert pwc_ref.cost_volume(one, one).shape[1] == 81


# =====================================================================================================================
# 1. cost volume forward
def _cv_call(lib, one, two, out, act, ws, splits):
    b, h, w, c = one.shape
    lib.call("ff_pwc_costvolume_fwd_ex", lib.p(one), lib.ld(one), lib.p(two), lib.ld(two), lib.p(out), lib.ld(out), b, h, w, c, act,
             lib.p(ws), splits, lib.stream())


@gpu
@pytest.mark.parametrize("case", R.CV_CASES, ids=R.cv_case_id)
def test_cost_volume_forward(lib, case, monkeypatch):
    ref = R.cv_reference(case)
    shape = (case.B, case.H, case.W, 81)
    want = {R.ACT_NONE: ref["vol"], R.ACT_LEAKY: F.leaky_relu(ref["vol"], 0.1)}
    for view in (False, True):
        guards = []
        one, two = put(ref["one"], view, guards), put(ref["two"], view, guards)
        for act in (R.ACT_NONE, R.ACT_LEAKY):
            for splits in R.cv_splits(case):
                what = f"{'view' if view else 'contiguous'} act {act} splits {splits}"
                # (a partial that the finish pass read without its having been written would carry the sentinel)
                ws = torch.full((splits * case.B * case.H * case.W * 81,), SENTINEL, device=DEV) if splits > 1 else None
                outs = []
                for _ in range(2):
                    buf, out = out_buf(shape, view, VOL_LEAD, LEVEL_WIDTH)
                    _cv_call(lib, one, two, out, act, ws, splits)
                    assert surroundings_kept(buf, out, VOL_LEAD), f"{what}: wrote outside channels [448, 529)"
                    outs.append(out)
                assert torch.equal(outs[0], outs[1]), f"{what}: the second call differs"
                R.check_bound("costvolume_fwd split" if splits > 1 else "costvolume_fwd unsplit", outs[0], want[act], ref["abs_vol"], case.C, what)
        assert untouched(guards), "an input buffer was written"
    # the product's own split decision
    notes = []
    real = lib.ops._timed_call

    def spy(label, name, *args, note=None):
        notes.append((name, note))
        return real(label, name, *args, note=note)

    monkeypatch.setattr(lib.ops, "_timed_call", spy)
    one, two = ref["one"].to(DEV), ref["two"].to(DEV)
    for act in (R.ACT_NONE, R.ACT_LEAKY):
        out = lib.pwc._cv_fwd(one, two, act=act)
        name, note = notes[-1]
        assert name == "ff_pwc_costvolume_fwd_ex" and note[1] == (case.B, case.H, case.W, case.C)
        assert note[2] == case.product_splits, f"_cv_fwd asked for {note[2]} splits, the table names {case.product_splits}"
        R.check_bound("costvolume_fwd split" if case.product_splits > 1 else "costvolume_fwd unsplit", out, want[act], ref["abs_vol"], case.C,
                      f"_cv_fwd act {act} ({note[2]} splits)")
    assert len(notes) == 2


@gpu
def test_entry_points_refuse_bad_arguments(lib):
    """FF_REQUIRE returns before any launch: C no multiple of 4, ld too small, splits without a workspace, H == 1 for backwarp."""
    err = lib.hip.FocusFlowHipError
    a, o = torch.zeros((1, 2, 2, 8), device=DEV), torch.zeros((1, 2, 2, 81), device=DEV)
    st, p = lib.stream(), lib.p
    with pytest.raises(err):
        lib.call("ff_pwc_costvolume_fwd_ex", p(a), 8, p(a), 8, p(o), 81, 1, 2, 2, 6, 0, p(None), 0, st)
    with pytest.raises(err):
        lib.call("ff_pwc_costvolume_fwd_ex", p(a), 8, p(a), 8, p(o), 80, 1, 2, 2, 8, 0, p(None), 0, st)
    with pytest.raises(err):
        lib.call("ff_pwc_costvolume_fwd_ex", p(a), 4, p(a), 8, p(o), 81, 1, 2, 2, 8, 0, p(None), 0, st)
    with pytest.raises(err):
        lib.call("ff_pwc_costvolume_fwd_ex", p(a), 8, p(a), 8, p(o), 81, 1, 2, 2, 8, 0, p(None), 2, st)
    with pytest.raises(err):
        lib.call("ff_pwc_costvolume_bwd", p(o), 80, p(a), 8, p(a), 8, 1, 2, 2, 8, st)
    with pytest.raises(err):
        lib.call("ff_pwc_gout_transpose", p(o), 81, p(o), 80, 1, 2, 2, st)
    fl = torch.zeros((1, 1, 4, 2), device=DEV)
    with pytest.raises(err):
        lib.call("ff_pwc_backwarp", p(a), 8, p(fl), 2, 1.0, p(a), 8, 1, 1, 4, 8, st)
    with pytest.raises(err):
        lib.call("ff_pwc_backwarp_bwd", p(a), 8, p(fl), 2, 1.0, p(a), 8, p(None), 8, p(None), 2, 1, 2, 2, 8, st)
    torch.cuda.synchronize()
    assert bool((o == 0).all()) and bool((a == 0).all())


# =====================================================================================================================
# 2. cost volume backward, gout_transpose, the autograd wrappers
@gpu
@pytest.mark.parametrize("case", R.CV_CASES, ids=R.cv_case_id)
def test_cost_volume_backward_and_transpose(lib, case):
    ref = R.cv_reference(case)
    b, h, w, c = case.B, case.H, case.W, case.C
    gt_want = R.gout_transpose_ref(ref["gy"])
    st = lib.stream()
    for g_ld in (81, 84):
        for view in (False, True):
            what = f"g_ld {g_ld} {'view' if view else 'contiguous'}"
            guards = []
            g = put(ref["gy"], g_ld == 84, guards, 0, 84)          # the first 81 channels of an 84-wide gradient: pads hold the sentinel
            one, two = put(ref["one"], view, guards), put(ref["two"], view, guards)
            assert lib.ld(g) == g_ld or h * w == 1
            grads, gts = [], []
            for _ in range(2):
                buf, grad = out_buf((b, h, w, c), view)
                lib.call("ff_pwc_costvolume_bwd", lib.p(g), g_ld, lib.p(two), lib.ld(two), lib.p(grad), lib.ld(grad), b, h, w, c, st)
                assert surroundings_kept(buf, grad, 4), f"{what}: grad one wrote outside its slice"
                grads.append(grad)
                tbuf, gt = out_buf((b, h, w, 81), view, 0, 84)     # as a view: the first 81 channels of an 84-wide tensor
                lib.call("ff_pwc_gout_transpose", lib.p(g), g_ld, lib.p(gt), 84 if view else 81, b, h, w, st)
                assert surroundings_kept(tbuf, gt, 0), f"{what}: gout_transpose wrote into the pad channels"
                gts.append(gt)
            assert torch.equal(grads[0], grads[1]) and torch.equal(gts[0], gts[1]), f"{what}: the second call differs"
            R.check_bound("costvolume_bwd", grads[0], ref["g_one"], ref["abs_g_one"], 81, f"{what}: grad one")
            assert torch.equal(gts[0].cpu(), gt_want), f"{what}: gout_transpose is not the permutation"
            buf, grad2 = out_buf((b, h, w, c), view)
            lib.call("ff_pwc_costvolume_bwd", lib.p(gts[0]), 84 if view else 81, lib.p(one), lib.ld(one), lib.p(grad2), lib.ld(grad2), b, h, w, c, st)
            assert surroundings_kept(buf, grad2, 4), f"{what}: grad two wrote outside its slice"
            R.check_bound("costvolume_bwd", grad2, ref["g_two"], ref["abs_g_two"], 81, f"{what}: grad two")
            assert untouched(guards), f"{what}: an input buffer (or a pad channel of the gradient) was written"


@gpu
@pytest.mark.parametrize("case", R.CV_CASES, ids=R.cv_case_id)
def test_cost_volume_autograd_wrappers(lib, case):
    ref = R.cv_reference(case)
    gy84 = torch.cat([ref["gy"], torch.full((*ref["gy"].shape[:3], 3), SENTINEL)], -1).to(DEV)
    wrappers = (("FunctionCorrelation", lib.pwc.FunctionCorrelation, 81), ("_CostVolume84", lib.pwcnet._CostVolume84.apply, 84))
    for name, fn, width in wrappers:
        for need_one, need_two in ((True, True), (True, False), (False, True)):
            what = f"{name} grads ({int(need_one)}, {int(need_two)})"
            one = ref["one"].to(DEV).requires_grad_(need_one)
            two = ref["two"].to(DEV).requires_grad_(need_two)
            out = fn(one, two)
            assert out.shape == (case.B, case.H, case.W, width)
            R.check_bound("costvolume_fwd split" if case.product_splits > 1 else "costvolume_fwd unsplit", out[..., :81], ref["vol"],
                          ref["abs_vol"], case.C, what)
            if width == 84:
                assert bool((out[..., 81:] == 0).all()), f"{what}: pad channels"
            out.backward(gy84[..., :width].contiguous())
            for t, need, key in ((one, need_one, "g_one"), (two, need_two, "g_two")):
                if need:
                    R.check_bound("costvolume_bwd", t.grad, ref[key], ref["abs_" + key], 81, f"{what}: {key}")
                else:
                    assert t.grad is None, f"{what}: {key} should be None"


# =====================================================================================================================
# 3. backwarp
def _bw_run(lib, x, flow, scale, gout, view):
    """Forward twice, backward twice with both pointers, once with each pointer alone; repeatability and guard bands are
    asserted here.  -> CPU tensors out, d_input, d_input (alone), d_flow (B, H, W, 2)."""
    b, h, w, c = x.shape
    guards = []
    xd, gd = put(x, view, guards), put(gout, view, guards)
    if view:
        fl = put(flow, True, guards, *FLOW_BUF)
    else:
        fl = flow.to(DEV)
    st = lib.stream()
    outs = []
    for _ in range(2):
        buf, out = out_buf((b, h, w, c), view)
        lib.call("ff_pwc_backwarp", lib.p(xd), lib.ld(xd), lib.p(fl), lib.ld(fl), float(scale), lib.p(out), lib.ld(out), b, h, w, c, st)
        assert surroundings_kept(buf, out, 4), "backwarp wrote outside its output slice"
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "backwarp: the second call differs"

    def backward(with_din, with_dflow):
        dbuf, din = out_buf((b, h, w, c), view, fill=0.0) if with_din else (None, None)
        dflow = torch.zeros((b, h, w, SLOT), device=DEV) if with_dflow else None
        lib.call("ff_pwc_backwarp_bwd", lib.p(xd), lib.ld(xd), lib.p(fl), lib.ld(fl), float(scale), lib.p(gd), lib.ld(gd), lib.p(din),
                 lib.ld(din) if with_din else 0, lib.p(dflow), SLOT, b, h, w, c, st)
        if with_din:
            assert surroundings_kept(dbuf, din, 4), "backwarp_bwd wrote outside d_input's slice"
        if with_dflow:
            assert bool((dflow[..., 2:] == 0).all()), "d_flow: channels >= 2 of the slot"
        return din, dflow

    din, dflow = backward(True, True)
    _, dflow2 = backward(True, True)
    din_alone, _ = backward(True, False)
    _, dflow_alone = backward(False, True)
    assert torch.equal(dflow, dflow2), "d_flow: the second call differs"
    assert torch.equal(dflow, dflow_alone), "d_flow with din == None differs"
    assert untouched(guards), "an input buffer was written"
    return outs[0].cpu(), din.cpu(), din_alone.cpu(), dflow[..., :2].cpu()


@gpu
@pytest.mark.parametrize("view", [False, True], ids=["contiguous", "view"])
@pytest.mark.parametrize("case", R.BW_CASES, ids=R.bw_case_id)
def test_backwarp_forward_and_backward(lib, case, view):
    ref = R.bw_reference(case)
    out, din, din_alone, dflow = _bw_run(lib, ref["x"], ref["flow"], case.scale, ref["gout"], view)
    tol, cid = ref["tol"], R.bw_case_id(case)
    assert bool((out[~ref["ex"]["valid"] & ref["keep"]] == 0).all()), "an invalid pixel is not exactly zero"
    R.check_rel(f"backwarp out {cid}", out, ref["out"], tol["out"], "out", ref["keep"])
    R.check_rel(f"backwarp d_input {cid}", din, ref["din"], tol["din"], "d_input")
    R.check_rel(f"backwarp d_input {cid}", din_alone, ref["din"], tol["din"], "d_input with dflow == None")
    assert bool((dflow[~ref["ex"]["valid"] & ref["keep"]] == 0).all()), "d_flow of an invalid pixel is not exactly zero"
    R.check_rel(f"backwarp d_flow {cid}", dflow, ref["dflow"], tol["dflow"], "d_flow", ref["keep_flow"])


@gpu
@pytest.mark.parametrize("view", [False, True], ids=["contiguous", "view"])
def test_backwarp_edge_inputs(lib, view):
    """Flow zero, whole-pixel shifts, the validity threshold, flows far outside: exact expectations, no outlier budget.  The
    tolerance is that of the random case of the same shape and flow_scale (the rounding of the sample position depends on the
    plane's size, the slope of the input on its distribution: both are the same here)."""
    case = R.EDGE_CASE
    tol = R.bw_reference(case)["tol"]
    x, gout = R.edge_data()
    every = torch.ones((case.B, case.H, case.W), dtype=torch.bool)
    # flow zero: every pixel valid, out = in
    out, din, _, dflow = _bw_run(lib, x, torch.zeros((case.B, case.H, case.W, 2)), case.scale, gout, view)
    assert bool((out != 0).all())
    R.check_rel("backwarp edge inputs", out, x.double(), tol["out"], "flow zero: out = in", every)
    R.check_rel("backwarp edge inputs", din, gout.double(), tol["din"], "flow zero: d_input = gout")
    # whole-pixel shifts
    for dx, dy in R.SHIFTS:
        flow = R.flow_for_offset(float(dx), float(dy))
        out, din, _, dflow = _bw_run(lib, x, flow, case.scale, gout, view)
        want, outside = R.shifted_input(x, dx, dy)
        assert int(outside.sum()) == case.H * case.W - (case.H - abs(dy)) * (case.W - abs(dx))
        assert bool((out[:, outside] == 0).all()), f"shift ({dx}, {dy}): a pixel whose source lies outside is not exactly zero"
        assert bool((dflow[:, outside] == 0).all()), f"shift ({dx}, {dy}): d_flow of such a pixel"
        R.check_rel("backwarp edge inputs", out, want.double(), tol["out"], f"shift ({dx}, {dy})", every)
        want_din = R.bw_oracle(x, flow, case.scale, gout, torch.float64)[1]
        R.check_rel("backwarp edge inputs", din, want_din, tol["din"], f"shift ({dx}, {dy}): d_input")
    # the validity threshold on the four borders
    flow, valid_px, invalid_px = R.threshold_input()
    want_out, want_din, _ = R.bw_oracle(x, flow, case.scale, gout, torch.float64)
    out, din, _, dflow = _bw_run(lib, x, flow, case.scale, gout, view)
    R.check_threshold_forward("backwarp edge inputs", out, want_out, valid_px, invalid_px, tol["out"])
    R.check_rel("backwarp edge inputs", out, want_out, tol["out"], "threshold input: every pixel", every)
    assert bool((dflow[:, invalid_px] == 0).all()), "threshold input: d_flow of an invalid pixel"
    R.check_rel("backwarp edge inputs", din, want_din, tol["din"], "threshold input: d_input")
    only_invalid = gout * invalid_px.view(1, case.H, case.W, 1)           # a gradient that reaches the invalid pixels only
    _, din, _, dflow = _bw_run(lib, x, flow, case.scale, only_invalid, view)
    assert bool((din == 0).all()) and bool((dflow == 0).all()), "threshold input: an invalid pixel contributes to a gradient"
    # far outside, in the four directions
    for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
        out, din, _, dflow = _bw_run(lib, x, R.flow_for_offset(1000.0 * sx, 700.0 * sy), case.scale, gout, view)
        assert bool((out == 0).all()) and bool((din == 0).all()) and bool((dflow == 0).all()), f"far outside ({sx}, {sy})"


# =====================================================================================================================
# 4. direct transposed convolution
@gpu
@pytest.mark.parametrize("case", R.DC_CASES, ids=R.dc_case_id)
def test_direct_transposed_convolution(lib, case):
    ref = R.dc_reference(case)
    wf = ref["wt"].permute(1, 0, 2, 3).flip(2, 3).contiguous().to(DEV)               # the equivalent forward conv's weight
    rows = torch.empty((case.Cout, 16 * case.Cin), device=DEV)
    lib.ops.pack_conv_weight(wf, rows, case.Cin, 0)
    rows_snap, bias = rows.clone(), ref["bias"].to(DEV)
    shape = (case.B, 2 * case.H, 2 * case.W, SLOT)
    for x_view in (False, True):
        for slot in (False, True):
            for with_bias in (True, False):
                what = f"x {'view' if x_view else 'full'} out {'slot' if slot else 'ld 16'} bias {int(with_bias)}"
                guards = []
                x = put(ref["x"], x_view, guards)
                outs = []
                for _ in range(2):
                    buf, out = out_buf(shape, slot, FLOW_LEAD, LEVEL_WIDTH)
                    lib.ops.deconv4x4s2_small(x, rows, bias if with_bias else None, case.Cout, out)
                    assert surroundings_kept(buf, out, FLOW_LEAD), f"{what}: wrote outside the slot"
                    assert bool((out[..., case.Cout:] == SENTINEL).all()), f"{what}: wrote channels >= Cout of the slot"
                    outs.append(out)
                assert torch.equal(outs[0], outs[1]), f"{what}: the second call differs"
                tag = "" if with_bias else "nobias_"
                R.check_bound("deconv4x4s2_small", outs[0][..., :case.Cout], ref[tag + "ref"], ref[tag + "abs"], 4 * case.Cin + 1, what)
                assert untouched(guards) and torch.equal(rows, rows_snap), f"{what}: an input buffer was written"
