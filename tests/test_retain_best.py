"""CPU tests of the per-image keypoint budget (sift_set_max_features): the numpy
rule of tests/retain_best_inputs.py against a literal restatement of
cv::KeyPointsFilter::retainBest, the properties of the inputs the GPU tests
(test_gpu_retain_best.py) rely on, and the new entry points at the ABI and in
the Python binding."""
import ctypes
import re

import numpy as np
import pytest

import retain_best_inputs as R
from test_abi import HEADER, declared_symbols

_cache = {}


def _sift(oracle, key, make):
    if key not in _cache:
        _cache[key] = oracle.sift(make())
    return _cache[key]


def _crafted():
    r = np.random.default_rng(11)
    base = (0.02 + r.random(40) * 0.2).astype(np.float32)
    return {
        "all_equal": np.full(17, 0.05, np.float32),
        "distinct": base,
        "pairs": np.repeat(base[:12], 2),
        "runs": np.repeat(base[:6], [1, 3, 18, 2, 1, 5]),           # one candidate with 18 peaks
        "shuffled_runs": r.permutation(np.repeat(base[:9], 4)),
        "neighbours": np.float32(0.03) + np.arange(9, dtype=np.float32) * np.float32(2 ** -29),  # last-bit steps
        "one": np.array([0.07], np.float32),
        "empty": np.zeros(0, np.float32),
    }


@pytest.mark.parametrize("name", list(_crafted()))
def test_rule_equals_sorted_restatement_on_crafted_vectors(name):
    v = _crafted()[name]
    k = len(v)
    for n in sorted({1, 2, max(k - 1, 1), k, k + 1, 3 * k + 7} | set(range(1, k + 2))):
        m = R.retain_best_mask(v, n)
        assert np.array_equal(m, R.retain_best_sorted(v, n)), (name, n)
        assert m.sum() >= min(n, k)
        if k > n:  # everything kept is >= everything dropped, and the n-th largest is the smallest kept
            assert v[m].min() == np.sort(v)[::-1][n - 1]
            assert not (~m).any() or v[~m].max() < v[m].min()
    assert R.retain_best_mask(v, 0).all()  # 0 = unlimited (the library's default)


def test_rule_cases_the_issue_names():
    eq = _crafted()["all_equal"]
    for n in (1, len(eq) - 1, len(eq), len(eq) + 1):
        assert R.retain_best_mask(eq, n).all()          # every response ties at the cut
    d = _crafted()["distinct"]
    for n in (1, len(d) - 1, len(d), len(d) + 5):
        assert R.retain_best_mask(d, n).sum() == min(n, len(d))


def test_rule_equals_sorted_restatement_on_random_vectors():
    r = np.random.default_rng(3)
    for trial in range(300):
        k = int(r.integers(1, 60))
        pool = (0.02 + r.random(int(r.integers(1, k + 1)))).astype(np.float32)
        v = pool[r.integers(0, len(pool), k)]            # many repeated values
        n = int(r.integers(1, k + 3))
        assert np.array_equal(R.retain_best_mask(v, n), R.retain_best_sorted(v, n)), (trial, k, n)


def test_response_bits_order_like_values():
    """The device compares the float bits as unsigned integers."""
    v = np.sort(np.concatenate([_crafted()["distinct"], _crafted()["neighbours"], [0.0, 0.02, 1e-38, 3e38]])
                .astype(np.float32))
    assert np.all(np.diff(v.view(np.uint32).astype(np.int64)) >= 0)


# ---- the GPU tests' inputs -----------------------------------------------------------
def test_batch_inputs_are_not_vacuous(oracle):
    """synth 0 and synth 2 at 97 x 131: 55 and 65 keypoints from 44 and 52
    candidates; the constant image has none.  The budgets of the batch case
    then cover K <= n, n < K, and a cut inside a multi-peak candidate."""
    got = []
    for seed in R.BATCH_SEEDS:
        kps, _ = _sift(oracle, ("synth", seed), lambda: oracle.synth_image(seed, *R.SHAPE))
        got.append((len(kps), R.distinct_candidates(kps)))
    assert got == [(55, 44), (65, 52)]
    assert len(oracle.sift(R.constant_image())[0]) == 0
    k0, _ = _sift(oracle, ("synth", 0), None)
    k2, _ = _sift(oracle, ("synth", 2), None)
    kept = {n: (int(R.retain_best_mask(k0["response"], n).sum()), int(R.retain_best_mask(k2["response"], n).sum()))
            for n in R.BATCH_N}
    assert kept[10000] == (55, 65) and kept[55] == (55, 55) and kept[10] == (10, 10)
    # n = 1: synth 0's strongest candidate has three orientation peaks; n = 56: the cut of synth 2 falls inside a pair
    assert kept[1] == (3, 1) and kept[56] == (55, 57)
    for kps, n in ((k0, 1), (k2, 56)):
        m = R.retain_best_mask(kps["response"], n)
        cut = m & (kps["response"] == kps["response"][m].min())
        assert cut.sum() > 1 and len(np.unique(R.candidate_ids(kps)[cut])) == 1   # one candidate straddles the cut
    # the host-path budgets (10, 40) cut synth 0
    assert all(R.retain_best_mask(k0["response"], n).sum() < 55 for n in (10, 40))


def test_tiled_input_has_ties_across_candidates(oracle):
    """np.tile(synth 5 at 64 x 64, (2, 2)): 66 keypoints from 59 candidates, 13
    response values shared by distinct candidates, 26 budgets that keep more
    than n -- some of them because distinct candidates tie at the cut."""
    kps, _ = _sift(oracle, "tiled", lambda: R.tiled_image(oracle))
    assert R.tiled_image(oracle).shape == R.TILED_SHAPE
    assert (len(kps), R.distinct_candidates(kps), int(R.candidate_ids(kps).max()) + 1) == (66, 59, 59)
    assert len(R.shared_response_values(kps)) == 13
    over = [n for n in range(1, len(kps)) if R.retain_best_mask(kps["response"], n).sum() > n]
    assert len(over) == 26
    ties = R.tie_budgets(kps)
    assert len(ties) >= 1 and set(ties) <= set(over)


# ---- the entry points ------------------------------------------------------------------
NEW = ["sift_set_max_features", "sift_multi_set_max_features"]


def test_header_declares_the_setters():
    assert set(NEW) <= set(declared_symbols())
    text = open(HEADER).read()
    assert re.search(r"int\s+sift_set_max_features\(sift_ctx\*\s*\w*,\s*int\s+n_per_image\);", text)
    assert re.search(r"int\s+sift_multi_set_max_features\(sift_multi\*\s*\w*,\s*int\s+n_per_image\);", text)


def test_library_exports_the_setters(siftgpu):
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    assert all(hasattr(L, s) for s in NEW)
    # a NULL context is SIFT_E_INVALID (no device needed)
    for s in NEW:
        f = getattr(L, s)
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]
        assert f(None, 5) == siftgpu.SIFT_E_INVALID


def test_python_methods_exist(siftgpu):
    assert callable(getattr(siftgpu.Context, "set_max_features", None))
    assert callable(getattr(siftgpu.MultiContext, "set_max_features", None))
