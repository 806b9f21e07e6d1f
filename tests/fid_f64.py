"""Test helper: the device tail of FID (sh-gan_amd/fid_stats.py ``frechet_device``) restated in float64 numpy, its yardstick, the case
generator and a numpy stand-in for the GEMM kernel.  Nothing here is shipped.

    fid = |mu_f - mu_r|^2 + tr sigma_f + tr sigma_r - 2 tr sqrt(sigma_f sigma_r)

``frechet_ns``: the trace from the coupled Newton-Schulz iteration on the non-symmetric product A = sigma_f sigma_r,

    s = |A|_F,  Y_0 = A / s,  Z_0 = I;   T = 1.5 I - 0.5 Z Y,  Y <- Y T,  Z <- T Z,  t_k = tr Y_k;   tr sqrt(A) = sqrt(s) t

THE STOPPING RULE, with d_k = |t_k - t_(k-1)| / |t_k| (NaN when t_k is 0 or not finite), tested in this order after step k = 1, 2, ...:
    1. d_k is not finite                              -> take t_(k-1), stop = 'turn'
    2. d_k <= tol (default 1e-10)                     -> take t_k,     stop = 'tol'
    3. k >= 2, d_k > d_(k-1) and d_(k-1) < 1e-3       -> take t_(k-1), stop = 'turn'
    4. k = max_iter (default 100) without a stop      -> raise
For a singular or nearly singular A the iteration converges as far as float64 allows and then turns round (the rounding noise in the
null space grows by 1.5 per step): rule 3 takes the trace before the turn; a fixed step count would run into the divergence.  A = 0 has the
square root 0 and takes no step.

``frechet_eigh``: the yardstick, by symmetric eigendecompositions alone (no iteration, no non-symmetric problem):
tr sqrt(sigma_f sigma_r) = sum sqrt(eig(sigma_f^(1/2) sigma_r sigma_f^(1/2))), eigenvalues clipped at 0."""
import math

import numpy as np

# (D, N, decay): the feature width, the rows, the spectrum's decay; N >= 4 D: a full-rank sigma, N < D: a rank-deficient one
SHAPES = [(40, 160, 3), (64, 256, 6), (64, 20, 6), (96, 400, 20), (96, 40, 8), (256, 2000, 16), (256, 100, 16)]
SEEDS = (0, 1, 2)
SEED_BASE = 100000
CASES = [(D, N, decay, seed) for D, N, decay in SHAPES for seed in SEEDS]
BOUND_FULL, BOUND_DEFICIENT = 1e-7, 1e-5        # relative to tr sigma_f + tr sigma_r, on the device (another summation order than numpy's)


def bound_of(D, N):
    if N >= 4 * D:
        return BOUND_FULL
    assert N < D, 'a case is either full-rank with N >= 4 D or rank-deficient with N < D'
    return BOUND_DEFICIENT


def _rotation(g, D):
    q, r = np.linalg.qr(g.standard_normal((D, D)))
    return q * np.sign(np.diag(r))


def features(D, N, decay, seed):
    """-> (fake, real) float64 [N, D]: randn(N, D) * exp(-decay * arange(D) / D) times a random orthogonal matrix; the fake side gets a
    0.3 randn(D) offset, the real side is scaled by 1.2 and uses a second rotation.

    The bounds are conditions on the inputs as much as on the code: when two random N-dimensional row spaces (N < D) meet at a small
    angle, sigma_f sigma_r has non-zero eigenvalues so small that the iteration has not resolved them when the rounding noise turns it
    round.  Over 12 seed bases x 3 seeds, ``frechet_ns`` in numpy was within 1.5e-8 (tr sigma_f + tr sigma_r) of ``frechet_eigh`` at (256, 100)
    in every draw, but at (64, 20) within 1.5e-8 in 6 bases of 12 and 1e-5 .. 4e-5 off in the others, and at (96, 40) between 1e-8 and 4.7e-6.
    ``SEED_BASE`` is one of the bases in which numpy stays within 1.5e-8 on all nine rank-deficient cases (tests/test_fid_tail_cpu.py
    asserts the bounds for numpy itself)."""
    g = np.random.RandomState(SEED_BASE + 1000 * D + 10 * N + seed)
    scale = np.exp(-decay * np.arange(D) / D)
    fake = (g.standard_normal((N, D)) * scale) @ _rotation(g, D) + 0.3 * g.standard_normal(D)
    real = 1.2 * (g.standard_normal((N, D)) * scale) @ _rotation(g, D)
    return fake, real


def stats(x):
    """-> (mu, sigma) of the rows of x, as FidStats.mean_cov defines them: sigma = x^T x / n - mu mu^T."""
    mu = x.mean(0)
    return mu, x.T @ x / len(x) - np.outer(mu, mu)


def case_stats(D, N, decay, seed):
    fake, real = features(D, N, decay, seed)
    return stats(fake) + stats(real)


def delta(t, t_prev):
    return abs(t - t_prev) / abs(t) if math.isfinite(t) and t != 0.0 else float('nan')


def frechet_ns(mu_f, sigma_f, mu_r, sigma_r, tol=1e-10, max_iter=100):
    """-> dict(fid, trace_sqrt, iterations, delta, stop), the fields of ``frechet_device``."""
    n = len(mu_f)
    base = float(np.square(mu_f - mu_r).sum() + np.trace(sigma_f) + np.trace(sigma_r))
    A = sigma_f @ sigma_r
    s = math.sqrt(float(np.sum(A * A)))
    if s == 0.0:
        return dict(fid=base, trace_sqrt=0.0, iterations=0, delta=0.0, stop='tol')
    eye = np.eye(n)
    Y, Z = A / s, eye.copy()
    t_prev, d_prev = float(np.trace(Y)), None
    for k in range(1, max_iter + 1):
        T = 1.5 * eye - 0.5 * (Z @ Y)
        Y, Z = Y @ T, T @ Z
        t = float(np.trace(Y))
        d = delta(t, t_prev)
        if not math.isfinite(d):
            taken, d_taken, stop = t_prev, d_prev, 'turn'
            break
        if d <= tol:
            taken, d_taken, stop = t, d, 'tol'
            break
        if d_prev is not None and d > d_prev and d_prev < 1e-3:
            taken, d_taken, stop = t_prev, d_prev, 'turn'
            break
        t_prev, d_prev = t, d
    else:
        raise RuntimeError(f'frechet_ns: no stop within {max_iter} steps (tr Y = {t!r}, delta = {d!r})')
    tr = math.sqrt(s) * taken
    return dict(fid=base - 2.0 * tr, trace_sqrt=tr, iterations=k, delta=d_taken, stop=stop)


def frechet_eigh(mu_f, sigma_f, mu_r, sigma_r):
    """-> (fid, tr sqrt(sigma_f sigma_r))."""
    w, V = np.linalg.eigh(sigma_f)
    root = (V * np.sqrt(np.clip(w, 0.0, None))) @ V.T
    M = root @ sigma_r @ root
    ev = np.linalg.eigvalsh((M + M.T) / 2)
    tr = float(np.sqrt(np.clip(ev, 0.0, None)).sum())
    return float(np.square(mu_f - mu_r).sum() + np.trace(sigma_f) + np.trace(sigma_r) - 2.0 * tr), tr


def numpy_matmul_fn(a, b, alpha=1.0, beta_diag=0.0, out=None, partials=None):
    """The stand-in for ``fid_stats.gemm_f64`` on CPU tensors, with numpy's products in the order ``frechet_ns`` forms them: out = alpha a b +
    beta_diag I per batch entry; partials [(batch,) 2, tiles]: the trace and the sum of squares in tile 0, zeros in the others."""
    import torch
    stacked = a.ndim == 3 or b.ndim == 3
    batch = max(a.shape[0] if a.ndim == 3 else 1, b.shape[0] if b.ndim == 3 else 1)
    n = a.shape[-1]
    if out is None:
        out = torch.empty((batch, n, n) if stacked else (n, n), dtype=torch.float64)
    eye = np.eye(n)
    for k in range(batch):
        x = (a[k] if a.ndim == 3 else a).numpy()
        y = (b[k] if b.ndim == 3 else b).numpy()
        c = alpha * (x @ y) + beta_diag * eye
        (out[k] if stacked else out).copy_(torch.from_numpy(c))
        if partials is not None:
            p = partials[k] if stacked else partials
            p.zero_()
            p[0, 0], p[1, 0] = float(np.trace(c)), float(np.sum(c * c))
    return out


def gemm_reference(a, b, alpha, beta_diag):
    """numpy float64 -> (c, bound): c = alpha a b + beta_diag I and the textbook entrywise bound (n + 2) 2^-53 (|alpha| |a| |b| + |beta_diag| I)
    for any order of the n products-and-sums, the scaling and the diagonal term."""
    n = a.shape[-1]
    c = alpha * (a @ b) + beta_diag * np.eye(n)
    return c, (n + 2) * 2.0 ** -53 * (abs(alpha) * (np.abs(a) @ np.abs(b)) + abs(beta_diag) * np.eye(n))
