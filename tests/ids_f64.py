"""The float64 yardstick of U-IDS / P-IDS (sh-gan_amd/ids_score.py): the features of the synthetic recipe, a plain numpy Newton-CG on

    f(w, b) = (|w|^2 + b^2) / 2 + C sum_i max(0, 1 - y_i (w.x_i + b))^2       (y = +1 reals, -1 fakes)

to a relative gradient norm of 1e-11, the two scores as CoModGAN defines them, and the numpy form of the streaming pass.  Nothing here is
shipped, and nothing here shares code with the product."""
import numpy as np

# (N, d, sep, seed) -> the scores this yardstick gives on the CPU (the issue's table)
CASES = {'A': (37, 24, 0.05, 1), 'B': (301, 130, 0.1, 1), 'C': (1030, 200, 0.1, 3), 'D': (1536, 512, 0.35, 3), 'E': (64, 2048, 0.1, 4)}
SCORES = {'A': (0.2568, 0.2432), 'B': (0.3272, 0.2193), 'C': (0.3471, 0.2437), 'D': (0.1175, 0.0293), 'E': (0.0, 0.0)}


def features(N, d, sep, seed):
    """-> (real, fake) float32 [N, d]: fake i is a noisy, shifted function of real i."""
    rs = np.random.RandomState(seed)
    mu = rs.standard_normal(d) / np.sqrt(d)
    real = (np.abs(rs.standard_normal((N, d))) * 0.5 + sep * mu).astype(np.float32)
    fake = (np.abs(rs.standard_normal((N, d))) * 0.5 - sep * mu + 0.3 * (real - 0.4)).astype(np.float32)
    return real, fake


def stack(real, fake):
    """-> (X~ [2N, d+1] float64 with the ones column, y [2N])."""
    X = np.concatenate([real, fake]).astype(np.float64)
    return np.concatenate([X, np.ones((X.shape[0], 1))], axis=1), np.concatenate([np.ones(len(real)), -np.ones(len(fake))])


def objective(v, Xt, y, C=1.0):
    m = np.maximum(0.0, 1.0 - y * (Xt @ v))
    return 0.5 * v @ v + C * (m @ m)


def gradient(v, Xt, y, C=1.0):
    m = np.maximum(0.0, 1.0 - y * (Xt @ v))
    return v - 2.0 * C * (Xt.T @ (y * m))


def fit(real, fake, C=1.0, tol=1e-11, max_newton=200):
    """-> (v [d+1] = (w, b), info): Newton-CG with a backtracking line search on f itself."""
    Xt, y = stack(real, fake)
    v = np.zeros(Xt.shape[1])
    g = gradient(v, Xt, y, C)
    g0 = np.linalg.norm(g)
    info = dict(newton=0, products=0, grad_norm0=g0)
    for _ in range(max_newton):
        gn = np.linalg.norm(g)
        if gn <= tol * g0:
            break
        act = (1.0 - y * (Xt @ v)) > 0
        Xa = Xt[act]
        hv = lambda u: u + 2.0 * C * (Xa.T @ (Xa @ u))        # noqa: E731
        s, r = np.zeros_like(v), -g.copy()
        p, rr = r.copy(), r @ r
        for _ in range(4 * len(v)):
            hp = hv(p)
            info['products'] += 1
            al = rr / (p @ hp)
            s += al * p
            r -= al * hp
            rn = r @ r
            if np.sqrt(rn) <= min(0.1, gn / g0) * 1e-2 * gn:
                break
            p = r + (rn / rr) * p
            rr = rn
        f0, t, slope = objective(v, Xt, y, C), 1.0, g @ s
        while objective(v + t * s, Xt, y, C) > f0 + 1e-4 * t * slope and t > 1e-12:
            t *= 0.5
        v = v + t * s
        g = gradient(v, Xt, y, C)
        info['newton'] += 1
    info['grad_norm'] = float(np.linalg.norm(g))
    info['converged'] = bool(info['grad_norm'] <= tol * g0)
    return v, info


def decisions(v, real, fake):
    Xt, _ = stack(real, fake)
    z = Xt @ v
    return z[:len(real)], z[len(real):]


def ids(v, real, fake):
    """-> (uids, pids, misclassified among the 2N, pairs won by the fake)."""
    dr, df = decisions(v, real, fake)
    errors, wins = int((dr <= 0).sum() + (df > 0).sum()), int((df > dr).sum())
    return errors / (2 * len(real)), wins / len(real), errors, wins


def pass_f64(x0, x1, v, mode, C=1.0, a=None, y=(1.0, -1.0)):
    """numpy form of ids_score.svm_pass on float32 rows: -> (q [D+2], z [n], a [n] uint8, bound_q [D+1], bound_z [n]); the bounds hold for
    any summation order: gamma_k * |X~|^T |s| with k = n + D + 4 for q, gamma_k * |X~| |v| with k = D + 2 for z."""
    X = np.asarray(x0, dtype=np.float64)
    yy = np.full(len(X), y[0])
    if x1 is not None:
        X = np.concatenate([X, np.asarray(x1, dtype=np.float64)])
        yy = np.concatenate([yy, np.full(len(x1), y[1])])
    Xt = np.concatenate([X, np.ones((len(X), 1))], axis=1)
    v = np.asarray(v, dtype=np.float64)
    z = Xt @ v
    if mode == 'grad':
        m = 1.0 - yy * z
        a = (m > 0).astype(np.uint8)
        s = -2.0 * C * yy * a * m
        loss = float((a * m * m).sum())
    else:
        s = 2.0 * C * np.asarray(a, dtype=np.float64) * z
        loss = 0.0
    q = np.concatenate([Xt.T @ s, [loss]])
    gamma = lambda k: k * 2.0 ** -53 / (1.0 - k * 2.0 ** -53)        # noqa: E731
    n, D = X.shape
    return q, z, a, gamma(n + D + 4) * (np.abs(Xt).T @ np.abs(s)), gamma(D + 2) * (np.abs(Xt) @ np.abs(v))


def torch_pass_fn(x0, x1, v, mode, C=1.0, a=None, y=(1.0, -1.0)):
    """``pass_fn`` for the product's fit on CPU tensors: ``pass_f64`` behind torch operands."""
    import torch
    q, z, a_out, _, _ = pass_f64(x0.numpy(), None if x1 is None else x1.numpy(), v.numpy(), mode, C, None if a is None else a.numpy(), y)
    return torch.from_numpy(q), torch.from_numpy(z), torch.from_numpy(np.asarray(a_out, dtype=np.uint8))
