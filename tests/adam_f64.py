"""Float64 restatement of the training tail (numpy only): gradient average -> sanitisation -> Adam, and the G_ema lerp.

The yardstick of tests/test_gpu_optim.py.  It states the formulas of ``torch.optim.Adam`` (weight_decay 0, amsgrad off) and of
``p.lerp(p_ema, beta)`` directly; tests/test_optim_cpu.py holds it against ``torch.optim.Adam`` run in float64 (``foreach=False``)."""
import numpy as np


def sanitize_f64(bucket, world=1):
    """bucket / world, then nan_to_num(nan=0, posinf=1e5, neginf=-1e5): NaN and the infinities are replaced, finite values kept."""
    g = np.asarray(bucket, np.float64) / float(world)
    g = np.where(np.isnan(g), 0.0, g)
    g = np.where(g == np.inf, 1e5, g)
    return np.where(g == -np.inf, -1e5, g)


def adam_step_f64(p, g, m, v, t, lr, beta1, beta2, eps):
    """One step for one parameter: (p, m, v, t) -> the same after the step with gradient g.  t: steps taken so far."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    t = t + 1
    m = beta1 * m + (1.0 - beta1) * g          # (exact for beta1 = 0, where m + (g - m) would round)
    v = beta2 * v + (1.0 - beta2) * g * g
    step_size = lr / (1.0 - beta1 ** t)
    denom = np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps
    return p - step_size * m / denom, m, v, t


def ema_f64(p_ema, p, beta):
    """``p.lerp(p_ema, beta)`` = p + beta * (p_ema - p)."""
    p_ema, p = np.asarray(p_ema, np.float64), np.asarray(p, np.float64)
    return p + beta * (p_ema - p)


def rel_err(a, b):
    """max |a - b| / max |b| of one tensor."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
