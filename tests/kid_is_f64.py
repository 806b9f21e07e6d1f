"""float64 yardsticks for KID, the Inception Score and the classifier head: plain numpy restatements of the two formulas of the reference
(lib/evaluator/stylegan_metrics/kernel_inception_distance.py:34-44 and inception_score.py:30-36), taking the subset index tables as
arguments instead of drawing them, and of softmax(feats @ W.T (+ b)).  Everything is evaluated in float64 whatever the inputs' dtype."""
import numpy as np


def kid_sums_f64(fake, real, idx_f, idx_r):
    """[S, 3]: per subset sum_{i != j} (x_i.x_j / n + 1)^3, the same for y, and sum_{i, j} (x_i.y_j / n + 1)^3 (lines 40-42: ``a.sum() -
    np.diag(a).sum()`` split into its x and y halves, and ``b.sum()``)."""
    fake, real = np.asarray(fake, dtype=np.float64), np.asarray(real, dtype=np.float64)
    n = real.shape[1]                                                   # line 34
    out = np.empty((len(idx_f), 3), dtype=np.float64)
    for s in range(len(idx_f)):
        x, y = fake[np.asarray(idx_f[s])], real[np.asarray(idx_r[s])]   # lines 38-39, the draws given
        axx = (x @ x.T / n + 1) ** 3                                    # line 40
        ayy = (y @ y.T / n + 1) ** 3
        b = (x @ y.T / n + 1) ** 3                                      # line 41
        out[s] = axx.sum() - np.diag(axx).sum(), ayy.sum() - np.diag(ayy).sum(), b.sum()
    return out


def kid_f64(fake, real, idx_f, idx_r):
    """Lines 36-43 with the draws given: t += (a.sum() - diag(a).sum()) / (m - 1) - b.sum() * 2 / m; kid = t / num_subsets / m."""
    sums = kid_sums_f64(fake, real, idx_f, idx_r)
    m = len(idx_f[0])
    t = 0.0
    for axx, ayy, b in sums:
        t += (axx + ayy) / (m - 1) - b * 2 / m                          # line 42
    return float(t / len(idx_f) / m)                                    # line 43


def is_f64(probs, num_splits):
    """inception_score.py:30-36 on probs [N, C] in dataset order -> (mean, std)."""
    probs = np.asarray(probs, dtype=np.float64)
    num_gen = probs.shape[0]
    scores = []
    for i in range(num_splits):
        part = probs[i * num_gen // num_splits: (i + 1) * num_gen // num_splits]       # line 32
        kl = part * (np.log(part) - np.log(np.mean(part, axis=0, keepdims=True)))      # line 33
        kl = np.mean(np.sum(kl, axis=1))                                               # line 34
        scores.append(np.exp(kl))                                                      # line 35
    return float(np.mean(scores)), float(np.std(scores))                               # line 36


def is_accumulator_f64(probs, splits, num_splits):
    """The [num_splits, C + 2] accumulator the product keeps: columns 0..C-1 = sum_i p_ic, column C = sum_i sum_c p_ic log p_ic (0 where
    p == 0), column C + 1 = the image count; images with a negative split are skipped."""
    probs = np.asarray(probs, dtype=np.float64)
    C = probs.shape[1]
    acc = np.zeros((num_splits, C + 2), dtype=np.float64)
    for p, s in zip(probs, np.asarray(splits)):
        if s < 0:
            continue
        acc[s, :C] += p
        nz = p > 0
        acc[s, C] += np.sum(p[nz] * np.log(p[nz]))
        acc[s, C + 1] += 1
    return acc


def softmax_head_f64(feats, w, b=None):
    """softmax(feats @ W.T (+ b)) over the classes, in float64."""
    z = np.asarray(feats, dtype=np.float64) @ np.asarray(w, dtype=np.float64).T
    if b is not None:
        z = z + np.asarray(b, dtype=np.float64)
    z = z - z.max(axis=1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=1, keepdims=True)
