"""The per-image keypoint budget (sift_set_max_features) written in numpy, and
the inputs its CPU and GPU tests share.

The rule is cv::KeyPointsFilter::retainBest: with K keypoints and a budget n,
K <= n keeps everything; otherwise T is the n-th largest response counted with
multiplicity and every keypoint with response >= T is kept -- at least n, more
when responses tie at the cut.  The library keeps the survivors in the unlimited
order, so the expected output of an image is always
`filter_keypoints(*oracle.sift(img), n)`.
"""
import numpy as np

import adversarial_inputs as A

SHAPE = (97, 131)         # the batch cases: synth 0, synth 2 and a constant image
BATCH_SEEDS = (0, 2)
BATCH_N = (1, 10, 44, 55, 56, 10000)
TILED_SHAPE = (128, 128)  # np.tile(synth 5 at 64 x 64, (2, 2)): equal responses on distinct candidates


def retain_best_mask(response, n):
    """Boolean mask of the keypoints the budget n keeps (n = 0: all)."""
    r = np.asarray(response, np.float32)
    k = len(r)
    if n <= 0 or k <= n:
        return np.ones(k, bool)
    t = np.partition(r, k - n)[k - n]  # the n-th largest
    return r >= t


def retain_best_sorted(response, n):
    """The same mask by a literal restatement of retainBest on a sorted copy:
    order by response, largest first; the boundary is element n - 1; the first n
    stay, and so does every later element >= the boundary."""
    r = np.asarray(response, np.float32)
    k = len(r)
    keep = np.zeros(k, bool)
    if not k > n:  # `if (n_points >= 0 && keypoints.size() > (size_t)n_points)`
        keep[:] = True
        return keep
    order = sorted(range(k), key=lambda i: -float(r[i]))
    boundary = r[order[n - 1]]
    keep[order[:n]] = True
    for i in order[n:]:
        if r[i] >= boundary:
            keep[i] = True
    return keep


def filter_keypoints(kps, desc, n):
    """(keypoints, descriptors) of one image under the budget n, in their own order."""
    m = retain_best_mask(kps["response"], n)
    return kps[m], desc[m]


def candidate_ids(kps):
    """Per keypoint, the index of the candidate (extremum) it came from: the
    orientation peaks of one candidate are consecutive and share every field
    but the angle."""
    if len(kps) == 0:
        return np.zeros(0, np.int64)
    f = np.stack([kps[k].view(np.int32) for k in ("x", "y", "size", "response", "octave")], 1)
    new = np.any(f[1:] != f[:-1], axis=1)
    return np.concatenate([[0], np.cumsum(new)])


def distinct_candidates(kps):
    """Distinct (x, y, size, response, octave) records.  Two extrema that
    refine to the same point give equal records (the reference removes no
    duplicates), so this can be below candidate_ids' count of slots: synth 0
    at 97 x 131 has 45 slots with 44 distinct records."""
    f = np.stack([kps[k].view(np.int32) for k in ("x", "y", "size", "response", "octave")], 1)
    return len(np.unique(f, axis=0))


def shared_response_values(kps):
    """Response values that more than one candidate has."""
    cid = candidate_ids(kps)
    first = np.concatenate([[True], cid[1:] != cid[:-1]]) if len(kps) else np.zeros(0, bool)
    vals, counts = np.unique(kps["response"][first], return_counts=True)
    return vals[counts > 1]


def tie_budgets(kps):
    """Budgets 1 <= n < K at which more than n keypoints are kept because
    distinct candidates tie at the cut."""
    r, cid = kps["response"], candidate_ids(kps)
    out = []
    for n in range(1, len(kps)):
        m = retain_best_mask(r, n)
        if m.sum() > n and len(np.unique(cid[m & (r == r[m].min())])) > 1:
            out.append(n)
    return out


def constant_image():
    return A.IMAGE_FAMILIES["constant"](*SHAPE)


def tiled_image(oracle):
    return np.ascontiguousarray(np.tile(oracle.synth_image(5, 64, 64), (2, 2)))
