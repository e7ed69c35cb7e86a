"""TEST INFRASTRUCTURE (not a test): the numpy float64 statement of the two-stage coupled Newton-Schulz iteration that
`dxmi_hip.ops.frechet_trace_sqrt` runs on the device -- the CPU model of the kernels' arithmetic, step for step:

    ns(M):  c = ||M||_F ; Y = M * (1 / c) ; Z = I
            repeat:  T = 1.5 I - 0.5 Z Y ;  Y <- Y T ;  Z <- T Z ;  tr_k = trace(Y) * sqrt(c)
            stop when |tr_k - tr_{k-1}| <= tol * |tr_k|  (converged; k >= 2: the first iterate has nothing to be compared with)
                 or tr_k not finite, or k = max_iters    (not converged)
            -> Y * sqrt(c) ~ M^(1/2)
    stage 1: R = ns(S1), R <- (R + R^T) / 2
    stage 2: M = R S2 R, M <- (M + M^T) / 2, tr sqrt(S1 S2) = trace(ns(M))

Only symmetric matrices are iterated on: the same iteration on the unsymmetric product S1 S2 overflows on ill-conditioned and
rank-deficient covariances."""
import numpy as np


def newton_schulz_sqrt(M, tol=1e-8, max_iters=100):
    """-> (Y * sqrt(c) ~ M^(1/2), trace of it, iterations, converged)."""
    n = M.shape[0]
    eye = np.eye(n)
    c = float(np.sqrt(np.sum(M * M)))
    Y = M * (1.0 / c)
    Z = eye.copy()
    rc = float(np.sqrt(c))
    prev, tr, k, ok = None, float("nan"), 0, False
    while k < max_iters:
        T = -0.5 * (Z @ Y) + 1.5 * eye
        Y, Z = Y @ T, T @ Z
        k += 1
        tr = float(np.trace(Y)) * rc
        if not np.isfinite(tr):
            break
        if prev is not None and abs(tr - prev) <= tol * abs(tr):
            ok = True
            break
        prev = tr
    return Y * rc, tr, k, ok


def frechet_trace_sqrt_model(sigma1, sigma2, tol=1e-8, max_iters=100):
    """tr sqrt(sigma1 sigma2) -> (trace, (k1, k2), converged).  k2 = 0 when stage 1 did not converge."""
    s1, s2 = np.asarray(sigma1, dtype=np.float64), np.asarray(sigma2, dtype=np.float64)
    R, _, k1, ok1 = newton_schulz_sqrt(s1, tol, max_iters)
    if not ok1:
        return float("nan"), (k1, 0), False
    R = 0.5 * (R + R.T)
    M = (R @ s2) @ R
    M = 0.5 * (M + M.T)
    _, tr, k2, ok2 = newton_schulz_sqrt(M, tol, max_iters)
    return tr, (k1, k2), ok2


def frechet_distance_model(mu1, sigma1, mu2, sigma2, tol=1e-8, max_iters=100):
    """The distance with the model's square-root trace -> (fid, (k1, k2), converged)."""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64), np.asarray(mu2, dtype=np.float64)
    tr, its, ok = frechet_trace_sqrt_model(sigma1, sigma2, tol, max_iters)
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr), its, ok
