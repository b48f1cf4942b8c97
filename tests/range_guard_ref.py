"""What tests/test_range_guard.py expects, written down without the code under test: the word ff_range_probe leaves, and the
table of the range guard's verdicts."""
import math

import numpy as np

X_LIMIT = 16376.0                      # csrc/ff_common.h: the fp16-split formats read |x| >= X_LIMIT as inf
INF_WORD = 0x7F800000
BELOW = float(np.nextafter(np.float32(X_LIMIT), np.float32(0)))       # the largest fp32 inside the range


def bits(v) -> int:
    """The int32 bits of an fp32 value."""
    return int(np.float32(v).view(np.int32))


def probe_word(x: np.ndarray, held: int = 0) -> int:
    """The word after ff_range_probe over the fp32 array `x`, which held `held` before: the bits of max|x| (non-negative floats
    order like their bit patterns), +inf for a NaN or an infinity anywhere, and never less than what it held."""
    a = np.abs(np.asarray(x, np.float32))
    return max(held, bits(a.max()) if np.isfinite(a).all() else INF_WORD)


# ---- the guard's verdicts -----------------------------------------------------------------------------------------------------
# route the forward took: "split" (the context features' convolutions on the fp16-split rows), "exact" (on the exact-fp32 rows:
# inference after the repair was armed), "recorded" (an autograd pass: split rows, armed or not)
ROUTES = ("split", "exact", "recorded")
QUIET = (False, False, "")
TAIL_FP32 = "Run this checkpoint / input with FF_CONV_PRECISION=fp32."
TAIL_ARMED = "exact-fp32 route from now on."
TAIL_RECORDED = "RECORDED"

IN_RANGE = (100.0, BELOW)
BEYOND = (X_LIMIT, 2 * X_LIMIT)             # finite and refused: the test is `not (m < X_LIMIT)`
NON_FINITE = (math.inf, math.nan)


def verdict_table():
    """Rows (m_ctx, m_fmap, route, (refuses, arms the exact route, tail of the message))."""
    rows = []
    for route in ROUTES:
        for m in IN_RANGE:                   # both inside: nothing to say, on any route
            rows += [(m, 100.0, route, QUIET), (100.0, m, route, QUIET)]
        for m in BEYOND + NON_FINITE:        # feature maps beyond the range have no repair; neither has an overflow INSIDE an encoder
            rows.append((100.0, m, route, (True, False, TAIL_FP32)))
        for m in NON_FINITE:
            rows.append((m, 100.0, route, (True, False, TAIL_FP32)))
        rows.append((2 * X_LIMIT, 2 * X_LIMIT, route, (True, False, TAIL_FP32)))
    for m in BEYOND:                         # a finite context output beyond the range: what the exact route exists for
        rows.append((m, 100.0, "split", (True, True, TAIL_ARMED)))        # that flow is lost, the next forward is right
        rows.append((m, BELOW, "exact", QUIET))                           # it took the exact route: its flow is right
        rows.append((m, 100.0, "recorded", (True, False, TAIL_RECORDED)))  # no exact route in a recorded pass
    return rows


def level_after(m_ctx, m_fmap, before=0.0):
    """The owner's running level once it has seen the pair."""
    m = math.inf if math.isnan(m_ctx) or math.isnan(m_fmap) else max(m_ctx, m_fmap)
    return max(before, m)
