"""Float64 numpy yardsticks of the training-run kernels (csrc/train_stats.hip, the health form of csrc/optim.hip): the moments table of
``training_stats.Collector``, the gradient-health figures of ``optim.ShgAdam(health=True)`` and the sample grid.  Plain restatements of the
definitions, written without looking at the kernels' reduction order; tolerances are derived where they are used."""
import numpy as np

EPS64 = 2.0 ** -52


def moments_f64(rows, slots):
    """rows: [(float32 array, slot)] in table order -> float64 [slots, 4] = {count, sum, sum of squares, non-finite count}."""
    acc = np.zeros([slots, 4], np.float64)
    for x, slot in rows:
        x = np.asarray(x, np.float32).reshape(-1)
        fin = np.isfinite(x)
        v = x[fin].astype(np.float64)
        acc[slot] += (fin.sum(), v.sum(), (v * v).sum(), (~fin).sum())
    return acc


def accumulate_fn(tab, acc, tensors):
    """``Collector(accumulate_fn=...)`` on the host: the call's table applied to ``acc`` (a CPU float64 tensor) with ``moments_f64``."""
    slots = [int(s) for s in np.asarray(tab)[:-1, 2]]
    add = moments_f64([(t.detach().cpu().numpy(), s) for t, s in zip(tensors.values(), slots)], acc.shape[0])
    import torch
    acc += torch.from_numpy(add).to(acc.device)


def sanitized_average_f32(raw, world, div_mode):
    """What the Adam pass makes of a bucket value, in float32 as the kernel does: -> (averaged, sanitised)."""
    raw = np.asarray(raw, np.float32)
    with np.errstate(all='ignore'):
        if div_mode == 1:
            avg = raw * np.float32(np.float32(1.0) / np.float32(world))
        elif div_mode == 2:
            avg = raw / np.float32(world)
        else:
            avg = raw.copy()
    return avg, np.nan_to_num(avg, nan=0.0, posinf=1e5, neginf=-1e5).astype(np.float32)


def health_f64(g_used, replaced, p_old, p_new):
    """The five figures of one segment and one step: g_used = the averaged, sanitised float32 gradient, replaced = how many elements the
    sanitisation replaced, p_old / p_new = the float32 parameter before / after."""
    g = np.asarray(g_used, np.float32).reshape(-1).astype(np.float64)
    po, pn = np.asarray(p_old, np.float32).reshape(-1), np.asarray(p_new, np.float32).reshape(-1)
    d = (po - pn).astype(np.float64)                    # the difference in float32, as the two stored values give it
    po = po.astype(np.float64)
    return np.array([(g * g).sum(), float(replaced), np.abs(g).max(), (po * po).sum(), (d * d).sum()], np.float64)


def image_grid_u8(img, grid_size, drange):
    """stylegan_default.py:75-84, restated."""
    lo, hi = drange
    img = (np.asarray(img, dtype=np.float32) - np.float32(lo)) * np.float32(255 / (hi - lo))
    img = np.rint(img).clip(0, 255).astype(np.uint8)
    gw, gh = grid_size
    _, C, H, W = img.shape
    return img.reshape(gh, gw, C, H, W).transpose(0, 3, 1, 4, 2).reshape(gh * H, gw * W, C)
