"""U-IDS and P-IDS, the unpaired / paired inception discriminative scores of CoModGAN (``metrics/inception_discriminative_score.py`` of its
TF code; the reference of this project does not ship the metric): a linear SVM is fitted to tell the detector features of the reals (y = +1)
from those of the fakes (y = -1), fake i being the completion of real i, and

    U-IDS = (#{reals: dec <= 0} + #{fakes: dec > 0}) / 2N          the SVM's error rate on its own training set (1 - ``svm.score``)
    P-IDS = mean_i [dec(fake_i) > dec(real_i)]                     the pairs in which the fake looks more real than its real

with dec(x) = w.x + b.  The fit minimises ``sklearn.svm.LinearSVC(dual=False)``'s objective (liblinear's L2R_L2LOSS_SVC: squared hinge, L2
penalty, the intercept a regularised extra feature of value 1)

    f(w, b) = (|w|^2 + b^2) / 2 + C sum_i max(0, 1 - y_i (w.x_i + b))^2

on float32 rows with every product and sum in float64.  f is 1-strongly convex: the optimum is unique and any solver that reaches it gives
the same numbers, so the solver is specified by its stopping rule, |grad f(w)| <= tol |grad f(0)|, not by its steps.

Deviation from the published pipeline: liblinear at sklearn's default ``tol=1e-4`` stops early (its coefficients are 3e-6 .. 4.5e-3 off
the optimum where ``tol=1e-12`` is within 4e-7); this module computes the optimum, which can move a published score by the samples nearest
the decision boundary.

The solver is a truncated Newton method on the generalised Hessian I + 2C X~_a^T X~_a (X~ = [X, 1], a = the rows with a positive hinge),
solved by conjugate gradients.  The gradient and every Hessian-vector product are one streaming pass of csrc/svm.hip over the two feature
matrices (``svm_pass``; they are never concatenated); the line search works on the n-vectors z = X~ w and X~ s alone (f along a ray is
piecewise quadratic in them).  There is no CPU path: host tensors raise, unless ``pass_fn`` replaces the kernel (CPU tests)."""
import math

import torch

from . import _lib, kernels
from ._lib import ShgError, check

MAX_D = 4096
_MODES = {'grad': 0, 'hv': 1}
CG_READ = 4                                 # conjugate-gradient steps between two host reads of the residual


def svm_pass(x0, x1, v, mode, C=1.0, a=None, y=(1.0, -1.0)):
    """One pass over the rows of ``x0`` [n0, D] (label y[0]) and ``x1`` [n1, D] | None (label y[1]): float32 HIP matrices with contiguous
    rows; a view with a row pitch larger than D is served as it is (no copy, no load past column D of a row).  ``v`` [D+1] float64.

    mode 'grad' -> (q [D+2], z [n0+n1], a [n0+n1] uint8): z = X~ v, a = [1 - y z > 0], q[:D+1] = X~^T s with s = -2C y a (1 - y z),
                   q[D+1] = the loss sum a (1 - y z)^2
    mode 'hv'   -> (q, z, a): ``a`` is the operand, z = X~ v, q[:D+1] = X~^T (2C a z), q[D+1] = 0

    Two launches on the current stream, no synchronisation, no atomics: the same bits on every run."""
    if mode not in _MODES:
        raise ShgError(f"svm_pass: mode must be 'grad' or 'hv' (got {mode!r})")
    launch = kernels._Launch()               # (``launch``, not ``L``: as diversity.pairwise_lpips, the allocation tests cover this function from
    x0 = launch.rows(x0, 'x0')               # tests/test_gpu_ids.py)
    x1 = launch.rows(x1, 'x1')
    v = launch.req(v, 'v', dtype=torch.float64)
    D = x0.shape[1]
    n0, n1 = x0.shape[0], (x1.shape[0] if x1 is not None else 0)
    if not 1 <= D <= MAX_D or n0 < 1 or (x1 is not None and (n1 < 1 or x1.shape[1] != D)):
        raise ShgError(f'svm_pass: row sets must be [n >= 1, D] with one D in 1..{MAX_D} (got {tuple(x0.shape)} and '
                       f'{tuple(x1.shape) if x1 is not None else None})')
    if v.ndim != 1 or v.shape[0] != D + 1:
        raise ShgError(f'svm_pass: v must be [{D + 1}] (got {tuple(v.shape)})')
    n = n0 + n1
    if mode == 'hv':
        a = launch.req(a, 'a', dtype=torch.uint8)
        if a is None or a.ndim != 1 or a.shape[0] != n:
            raise ShgError(f"svm_pass: mode 'hv' needs a [{n}] uint8 (the active rows of a 'grad' pass)")
    elif a is not None:
        raise ShgError("svm_pass: mode 'grad' writes a; it takes none")
    lib = _lib.get_lib()
    nbytes = int(lib.shg_svm_pass_workspace_bytes(n0, n1, D))
    ws = launch.new((max(1, nbytes // 8),), dtype=torch.float64)
    q = launch.new((D + 2,), dtype=torch.float64)
    z = launch.new((n,), dtype=torch.float64)
    if mode == 'grad':
        a = launch.new((n,), dtype=torch.uint8)
    ld = lambda t: t.stride(0) if t.shape[0] > 1 else max(t.stride(0), D)        # noqa: E731  (a single row has no pitch to speak of)
    with launch:
        check(lib.shg_svm_pass_f64(kernels._ptr(x0), n0, ld(x0), float(y[0]), kernels._ptr(x1), n1, ld(x1) if x1 is not None else 0, float(y[1]),
                                   D, _MODES[mode], float(C), kernels._ptr(v), kernels._ptr(z), kernels._ptr(a), kernels._ptr(q), kernels._ptr(ws),
                                   nbytes, launch.stream()), 'svm_pass')
    return q, z, a


def _dot(u, w):
    return (u * w).sum()                     # (an elementwise product and torch's own reduction: no BLAS handle for a [D+1] vector)


def _check_features(real, fake, what, need_device):
    for t, name in ((real, 'real'), (fake, 'fake')):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.ndim != 2 or not t.is_contiguous():
            raise ShgError(f'{what}: {name} must be a contiguous float32 tensor [N, D]')
    if real.shape != fake.shape or real.device != fake.device:
        raise ShgError(f'{what}: real and fake must have one shape and one device: fake i is the completion of real i (got '
                       f'{tuple(real.shape)} on {real.device} and {tuple(fake.shape)} on {fake.device})')
    if real.shape[0] < 1 or not 1 <= real.shape[1] <= MAX_D:
        raise ShgError(f'{what}: need N >= 1 rows of 1..{MAX_D} features (got {tuple(real.shape)})')
    if need_device and not real.is_cuda:
        raise ShgError(f'{what}: the features must reside on a HIP (cuda) device: libshgan_hip has no CPU path')


def _line_search(w, s, z, zs, y, C, max_iter=40):
    """The minimiser of phi(alpha) = f(w + alpha s) along a descent direction, from the n-vectors z = X~ w and zs = X~ s alone: phi' is
    piecewise linear and increasing, so a Newton iteration on it, kept inside the bracket [phi' < 0, phi' > 0], ends in a few steps.  One
    host read of (phi', phi'') per step."""
    ws, ss, yzs = _dot(w, s), _dot(s, s), y * zs

    def slope(alpha):
        m = 1.0 - y * (z + alpha * zs)
        on = (m > 0).to(torch.float64)
        d1 = ws + alpha * ss - 2.0 * C * _dot(on * m, yzs)
        d2 = ss + 2.0 * C * _dot(on * zs, zs)
        return torch.stack([d1, d2]).tolist()
    d0 = slope(0.0)[0]
    if not d0 < 0.0:                         # (not a descent direction: rounding at the optimum)
        return 0.0
    lo, hi, alpha = 0.0, None, 1.0
    for _ in range(max_iter):
        d1, d2 = slope(alpha)
        if abs(d1) <= 1e-8 * abs(d0):
            break
        if d1 < 0.0:
            lo = alpha
        else:
            hi = alpha
        nxt = alpha - d1 / d2
        if not nxt > lo or (hi is not None and not nxt < hi):
            nxt = 2.0 * alpha if hi is None else 0.5 * (lo + hi)
        if nxt == alpha:
            break
        alpha = nxt
    return alpha


def fit_linear_svc(real, fake, C=1.0, tol=1e-9, max_newton=100, pass_fn=None):
    """real, fake [N, D] float32 (HIP tensors; any device with ``pass_fn``) -> dict(w float64 [D], b, grad_norm, grad_norm0, newton_iters,
    passes, converged): the minimiser of f (module docstring) to |grad f(w, b)| <= tol |grad f(0)|, or ``converged=False`` after
    ``max_newton`` Newton steps.  ``pass_fn(x0, x1, v, mode, C=, a=)`` replaces ``svm_pass``.  The conjugate-gradient scalars stay on the
    device: the host reads the residual every ``CG_READ`` steps (a solve may run up to ``CG_READ - 1`` products past its target) and (phi', phi'')
    per line-search step."""
    _check_features(real, fake, 'fit_linear_svc', pass_fn is None)
    run = pass_fn if pass_fn is not None else svm_pass
    C, tol = float(C), float(tol)
    if not C > 0 or not tol > 0 or int(max_newton) < 0:
        raise ShgError(f'fit_linear_svc: need C > 0, tol > 0 and max_newton >= 0 (got {C}, {tol}, {max_newton})')
    N, D = real.shape
    launch = kernels._Launch()
    launch.view(real, 'real')
    y = launch.new((2 * N,), torch.float64)
    y[:N] = 1.0
    y[N:] = -1.0
    w = launch.new((D + 1,), torch.float64).zero_()
    passes = newton = 0
    gnorm0 = None
    while True:
        q, z, a = run(real, fake, w, 'grad', C=C)
        passes += 1
        g = w + q[:D + 1]
        gnorm = float(torch.linalg.vector_norm(g))
        if gnorm0 is None:
            gnorm0 = gnorm
        if not math.isfinite(gnorm):
            raise ShgError(f'fit_linear_svc: the gradient norm is {gnorm} after {newton} Newton steps (non-finite features?)')
        if gnorm <= tol * gnorm0 or newton >= int(max_newton):
            break
        # conjugate gradients on (I + 2C X~_a^T X~_a) s = -g, to a residual that shrinks with the gradient (superlinear outer convergence)
        eta = min(0.1, math.sqrt(gnorm / gnorm0))
        eta = max(eta, 0.1 * tol * gnorm0 / gnorm)
        s, zs = launch.new((D + 1,), torch.float64).zero_(), launch.new((2 * N,), torch.float64).zero_()
        r = -g
        p, rr = r.clone(), _dot(r, r)        # rr, alpha and beta stay on the device; the host reads the residual every CG_READ steps
        limit = max(10, min(2 * (D + 1), 1000))
        for k in range(limit):
            qp, zp, _ = run(real, fake, p, 'hv', C=C, a=a)
            passes += 1
            hp = p + qp[:D + 1]
            php = _dot(p, hp)
            alpha = torch.where(php > 0, rr / php, 0.0)       # (p = 0 once the residual is exactly 0: the steps up to the next read add nothing)
            s.addcmul_(p, alpha)
            zs.addcmul_(zp, alpha)
            r.addcmul_(hp, -alpha)
            rr_new = _dot(r, r)
            if k % CG_READ == CG_READ - 1 or k == limit - 1:
                res, curv = torch.stack([rr_new, php]).tolist()
                if not curv > 0.0 or not math.sqrt(res) > eta * gnorm:
                    break
            p = r + torch.where(rr > 0, rr_new / rr, 0.0) * p
            rr = rr_new
        step = _line_search(w, s, z, zs, y, C)
        if step == 0.0:                      # no progress is possible in float64: report what was reached
            break
        w = w + step * s
        newton += 1
    return dict(w=w[:D].clone(), b=float(w[D]), grad_norm=gnorm, grad_norm0=gnorm0, newton_iters=newton, passes=passes,
                converged=bool(gnorm <= tol * gnorm0))


def ids_from_features(real, fake, C=1.0, tol=1e-9, max_newton=100, pass_fn=None):
    """real, fake [N, D] contiguous float32 HIP tensors of one shape, fake i the completion of real i -> dict(uids, pids, uids_errors (the
    misclassified among the 2N), pids_wins (the pairs with dec(fake) > dec(real)), n, dec (float64 [2N]: the decisions, reals then fakes), and
    the fields of ``fit_linear_svc``).  The decisions
    are the z of one last 'grad' pass at the fitted (w, b).  A fit that did not converge raises ``ShgError``: there is no silent score."""
    fit = fit_linear_svc(real, fake, C=C, tol=tol, max_newton=max_newton, pass_fn=pass_fn)
    if not fit['converged']:
        raise ShgError(f"ids_from_features: the SVM fit did not converge in {fit['newton_iters']} Newton steps ({fit['passes']} passes): gradient "
                       f"norm {fit['grad_norm']:.6e}, needed <= tol * |grad f(0)| = {tol:g} * {fit['grad_norm0']:.6e}")
    N = real.shape[0]
    v = torch.cat([fit['w'], fit['w'].new_tensor([fit['b']])])
    _, z, _ = (pass_fn if pass_fn is not None else svm_pass)(real, fake, v, 'grad', C=float(C))
    dec_real, dec_fake = z[:N], z[N:]
    errors = int((dec_real <= 0).sum() + (dec_fake > 0).sum())
    wins = int((dec_fake > dec_real).sum())
    return dict(fit, uids=errors / (2 * N), pids=wins / N, uids_errors=errors, pids_wins=wins, n=N, dec=z, passes=fit['passes'] + 1)
