"""The host forms of the four segmented matchers copy back the live rows only.

sift_knn_match_l1_segmented, _l1_u8_segmented, _l2sqr_u8_segmented and
sift_knn_match_window_segmented (one case per metric) share one copy-back:
rows [clamp(q_offsets[0]), clamp(q_offsets[n])) of idx / dist come back, every
other row of the caller's arrays keeps what the caller put there.  One shape
for all: 3 segments, q_cap 300 (more than one query tile of every matcher: 64,
256, 128), t_cap 200, q_offsets [5, 5, 140, 330] -- an empty segment, a first
offset above 0 and a last offset above q_cap -- with k 1 and 2, a shared train
set and train offsets.  The C entry points are called directly, so that the
sentinel is the caller's and not the Python wrapper's own -1 / +inf fill.
References: oracle/match.py and the integer references of match_u8_inputs.py /
match_l2_inputs.py (through match_window_inputs.dense_seg_ref), and
match_window_inputs.window_ref; every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_bits_equal

import match_window_inputs as W

pytestmark = pytest.mark.gpu

Q_CAP, T_CAP = 300, 200
Q_OFF = np.array([5, 5, 140, 330], np.int32)
T_OFF = np.array([0, 60, 60, 200], np.int32)      # segment 1 is empty on the query side, segment 2 has 140 train rows
LO, HI = 5, Q_CAP
EXTRA = 16      # sentinel rows after every output
DENSE = ["sift_knn_match_l1_segmented", "sift_knn_match_l1_u8_segmented", "sift_knn_match_l2sqr_u8_segmented"]
FORMS = [(m, False) for m in range(3)] + [(m, True) for m in range(3)]
FORM_IDS = W.METRIC_IDS + ["window_" + i for i in W.METRIC_IDS]


@functools.lru_cache(maxsize=None)
def _inputs(metric):
    rng = np.random.default_rng(20 + metric)
    q, t = W.rows_of(rng, Q_CAP, metric), W.rows_of(rng, T_CAP, metric)
    qk = W.kpts_at(rng.random((Q_CAP, 2)) * [W.COLS, W.ROWS])
    tk = W.kpts_at(rng.random((T_CAP, 2)) * [W.COLS, W.ROWS])
    for a in (q, t, qk, tk):
        a.setflags(write=False)
    return q, t, qk, tk


@functools.lru_cache(maxsize=None)
def _reference(metric, window, seg_train, k):
    q, t, qk, tk = _inputs(metric)
    toff = T_OFF if seg_train else None
    if window:
        return W.window_ref(metric, q, qk, Q_OFF, t, tk, toff, W.RADIUS, k=k)[:2]
    return W.dense_seg_ref(metric, q, Q_OFF, t, toff, k)


@pytest.mark.parametrize("seg_train", [False, True], ids=["shared", "segmented"])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("metric,window", FORMS, ids=FORM_IDS)
def test_host_form_copies_back_the_live_rows_only(ctx, metric, window, k, seg_train):
    q, t, qk, tk = _inputs(metric)
    pint = ctypes.POINTER(ctypes.c_int)
    pf = ctypes.POINTER(ctypes.c_float)
    idx = np.full((Q_CAP + EXTRA, k), W.SENT_I, np.int32)
    dist = np.full((Q_CAP + EXTRA, k), W.SENT_F, np.float32)
    qo = Q_OFF.ctypes.data_as(pint)
    to = T_OFF.ctypes.data_as(pint) if seg_train else None
    rows = (lambda a: a.ctypes.data_as(pf)) if metric == W.L1_F32 and not window else (lambda a: a.ctypes.data)
    out = (idx.ctypes.data_as(pint), dist.ctypes.data_as(pf))
    if window:
        rc = ctx._L.sift_knn_match_window_segmented(ctx.h, metric, rows(q), qk.ctypes.data, qo, 3, Q_CAP, rows(t),
                                                    tk.ctypes.data, to, T_CAP, None, None, float(W.RADIUS), W.ROWS,
                                                    W.COLS, k, *out)
    else:
        rc = getattr(ctx._L, DENSE[metric])(ctx.h, rows(q), qo, 3, Q_CAP, rows(t), to, T_CAP, k, *out)
    assert rc == 0, rc
    ri, rd = _reference(metric, window, seg_train, k)
    what = f"{FORM_IDS[metric + 3 * window]} k={k} seg_train={seg_train}"
    assert_bits_equal(idx[LO:HI], ri[LO:HI], what + " idx, live rows")
    assert_bits_equal(dist[LO:HI], rd[LO:HI], what + " dist, live rows")
    dead = np.r_[0:LO, HI:Q_CAP + EXTRA]
    assert (idx[dead] == W.SENT_I).all() and (dist[dead] == W.SENT_F).all(), what + ": rows outside [5, 300) written"
