"""numpy restatement of the cost-GMM threshold of ``DinoDetrSSOD._fit_gmm`` (detr_ssod/models/dino_detr_ssod.py:832-890):
a two-component, one-feature ``sklearn.mixture.GaussianMixture(2, weights_init=[.5, .5], means_init=[min, max],
precisions_init=[[1], [1]], covariance_type='diag', reg_covar=1e-5)`` fit, then ``predict`` / ``score_samples`` and the
threshold pick.  It follows the dtype flow of scikit-learn 1.7.2 (mixture/_base.py, _gaussian_mixture.py) step by step, so
that a fixture recorded from sklearn is reproduced exactly in threshold, labels and iteration count:

* X stays float32: ``X ** 2`` / ``X * X`` are rounded to fp32 before they meet the fp64 parameters;
* ``means_init`` is built from two float32 scalars, so it is a float32 array: the first E-step squares the means in fp32;
* ``log(2 pi)`` is cast to X's dtype (fp32) before it is added;
* ``nk = sum(resp) + 10 eps(f64)``, ``cov = avg_X2 - means**2 + reg_covar``, ``weights /= weights.sum()``,
  ``precisions_chol = 1 / sqrt(cov)``, ``precisions = precisions_chol ** 2``;
* logsumexp as scipy 1.15 computes it for two terms: ``log1p(exp(min - max)) + max``;
* the sums and dot products are numpy's own calls on sklearn's array shapes, so they round as there.

It also returns the *deciding margin* of the discrete results (how close a label, the convergence test or the threshold
pick came to flipping), so that a comparison against an implementation with a different summation order can tell a real
disagreement from a rounding-level tie.
"""
import numpy as np

EPS10 = 10.0 * np.finfo(np.float64).eps


def _weighted_log_prob(X, means, prec_chol, weights):
    """(n, 2) fp64 = _estimate_log_gaussian_prob (diag) + log(weights), with sklearn's array shapes and numpy calls, so the
    products and sums round exactly as there.  X (n, 1) fp32; means (2, 1) fp32 before the first M-step, fp64 after."""
    precisions = prec_chol ** 2
    log_prob = (np.sum((means ** 2 * precisions), 1) - 2.0 * np.dot(X, (means * precisions).T)
                + np.dot(X ** 2, precisions.T))
    log_det = np.sum(np.log(prec_chol), axis=1)
    return -0.5 * (1 * np.log(2 * np.pi).astype(X.dtype) + log_prob) + log_det + np.log(weights)


def _lse2(w):
    hi, lo = np.maximum(w[:, 0], w[:, 1]), np.minimum(w[:, 0], w[:, 1])
    return np.log1p(np.exp(lo - hi)) + hi


def fit_gmm_ref64(costs, reg_covar=1e-5, tol=1e-3, max_iter=100):
    """costs: 1-D array of fp32 costs (any order).  Returns dict(thr (np.float32), labels (int64, in the order of the
    sorted costs), scores (fp64, sorted order), n_iter, converged, margin, x (the sorted fp32 costs), error)."""
    x = np.sort(np.asarray(costs, np.float32).reshape(-1), kind="stable")
    n = x.size
    if n == 0:
        return dict(thr=np.float32(0.0), labels=np.zeros(0, np.int64), scores=np.zeros(0), n_iter=0, converged=False,
                    margin=np.inf, x=x, error=False)
    if n == 1:
        return dict(thr=x[0], labels=np.zeros(1, np.int64), scores=np.zeros(1), n_iter=0, converged=False,
                    margin=np.inf, x=x, error=False)
    X = x.reshape(-1, 1)
    means = np.array([x.min(), x.max()]).reshape(2, 1)             # float32, as _fit_gmm builds means_init
    prec_chol = np.sqrt(np.array([1.0, 1.0]).reshape(2, 1))
    weights = np.array([0.5, 0.5])
    lower = -np.inf
    margin = np.inf
    converged = False
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        prev = lower
        w = _weighted_log_prob(X, means, prec_chol, weights)
        lpn = _lse2(w)
        resp = np.exp(w - lpn[:, np.newaxis])
        nk = resp.sum(axis=0) + EPS10
        means = np.dot(resp.T, X) / nk[:, np.newaxis]
        cov = np.dot(resp.T, X * X) / nk[:, np.newaxis] - means ** 2 + reg_covar
        if np.any(np.less_equal(cov, 0.0)):
            return dict(thr=np.float32(np.nan), labels=np.zeros(n, np.int64), scores=np.full(n, np.nan), n_iter=n_iter,
                        converged=False, margin=0.0, x=x, error=True)
        weights = nk / nk.sum()
        prec_chol = 1.0 / np.sqrt(cov)
        lower = np.mean(lpn)
        change = lower - prev
        margin = min(margin, abs(abs(change) - tol))
        if abs(change) < tol:
            converged = True
            break
    w = _weighted_log_prob(X, means, prec_chol, weights)
    labels = w.argmax(axis=1).astype(np.int64)
    scores = _lse2(w)
    margin = min(margin, float(np.min(np.abs(w[:, 1] - w[:, 0]) / np.maximum(1.0, np.abs(w).max(1)))))
    comp = 0 if (labels == 0).any() else 1
    idx = np.nonzero(labels == comp)[0]
    s, xv = scores[idx], x[idx]
    b = int(np.argmax(s))                            # first maximum = the smallest cost (x is sorted ascending)
    best = idx[b]
    other = s[xv != xv[b]]
    if other.size:
        margin = min(margin, float(s[b] - other.max()) / max(1.0, abs(float(s[b]))))
    return dict(thr=x[best], labels=labels, scores=scores, n_iter=n_iter, converged=converged, margin=margin, x=x,
                error=False)


def double_filter_sets(match_cost, match_inds, gt_scores, thr, base_thr=0.4):
    """Step 4 of the unsupervised loss for one image: (keep_base, keep_gmm | keep_base), sorted unique int64 indices.
    Comparisons are fp32 (the cost tensor against a fp32 threshold, the scores against fp32(base_thr))."""
    match_cost = np.asarray(match_cost, np.float32)
    keep_gmm = np.asarray(match_inds, np.int64)[match_cost <= np.float32(thr)]
    keep_base = np.nonzero(np.asarray(gt_scores, np.float32) >= np.float32(base_thr))[0].astype(np.int64)
    return np.unique(keep_base), np.unique(np.concatenate([keep_gmm, keep_base]))
