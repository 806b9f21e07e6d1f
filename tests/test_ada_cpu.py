"""The ADA pipe without a GPU: the float64 restatement (tests/ada_f64.py, the yardstick of tests/test_gpu_ada.py) checked on the cases whose
answer is known in closed form, the controller's arithmetic on CPU tensors, and what the public interface refuses."""
import numpy as np
import pytest
import torch

import ada_f64 as R


def _reflect_extended(x, dy, dx):
    """out[y, x] = x_reflect[y + dy, x + dx] (whole-sample reflection, no edge repeat)."""
    H, W = x.shape[-2:]

    def fold(i, n):
        i = np.abs(i)
        return np.where(i > n - 1, 2 * (n - 1) - i, i)
    iy, ix = fold(np.arange(H) + dy, H), fold(np.arange(W) + dx, W)
    return x[..., iy, :][..., ix]


def test_restatement_identity_returns_its_input():
    x = torch.from_numpy(np.random.RandomState(0).standard_normal((2, 3, 16, 24)))
    y, m = R.geometry(x, R.affine('identity', 2, 16, 24))
    assert m == (6, 6, 6, 6)
    err = float((y - x).abs().max())
    print(f'identity: max |y - x| = {err:.2e}')
    assert err <= 1e-10


def test_restatement_integer_translation_shifts_reflect_extended_pixels():
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((2, 3, 16, 24)))
    y, m = R.geometry(x, R.affine('shift', 2, 16, 24))               # translate2d(3, -2): out(o) = in(o + (3, -2))
    assert m == (3, 8, 9, 4)
    want = _reflect_extended(x.numpy(), -2, 3)
    err = float(np.abs(y.numpy() - want).max())
    print(f'integer shift: max error = {err:.2e}')
    assert err <= 1e-10


def test_restatement_zoom_out_clamps_margins_and_pads_with_exact_zeros():
    x = torch.from_numpy(np.random.RandomState(2).standard_normal((1, 2, 16, 24)))
    smp = []
    y, m = R.geometry(x, R.affine('zoom_out4', 1, 16, 24), samples=smp)
    assert m == (23, 15, 23, 15)
    # sample j of the x2 grid sits at source coordinate 4 * (j - size - 5) / 2 from the centre, i.e. at pixel 2 * that - 0.5 + (U - 1) / 2 of
    # the upsampled padded image (U = 2 * (size + 2 * margin) pixels); bilinear reads nothing at or below -1 and at or above U
    S = smp[0]
    assert tuple(S.shape) == (1, 2, 44, 60)
    for axis, size, margin in ((3, 24, 23), (2, 16, 15)):
        U = 2 * (size + 2 * margin)
        j = np.arange(2 * size + 12)
        px = 2 * (4 * (j - size - 5) / 2) - 0.5 + (U - 1) / 2
        out = (px <= -1) | (px >= U)
        assert out.sum() >= 8 and (~out).sum() >= 16
        idx = torch.from_numpy(np.nonzero(out)[0])
        assert float(S.index_select(axis, idx).abs().max()) == 0.0
    assert float(y.abs().max()) > 0.05 and bool(torch.isfinite(y).all())


def test_restatement_gates_closed_at_p_zero():
    rs = np.random.RandomState(3)
    u, g = torch.from_numpy(rs.uniform(size=(8, 24))), torch.from_numpy(rs.standard_normal((8, 8)))
    cfg = {k: 1 for k in R.GEOM_KEYS + R.COLOR_KEYS}
    pr = R.params(u, g, 0.0, cfg, 16, 24, torch.float64)
    assert torch.equal(pr['G_inv'], torch.eye(3, dtype=torch.float64).expand(8, 3, 3))
    assert torch.equal(pr['C'], torch.eye(4, dtype=torch.float64)[:3].expand(8, 3, 4))
    pr1 = R.params(u, g, 1.0, cfg, 16, 24, torch.float64)
    assert not torch.equal(pr1['G_inv'], pr['G_inv']) and not torch.equal(pr1['C'], pr['C'])


def test_restatement_adjoint_and_second_order_are_consistent():
    """<A x, w> = <x, A^T w> and d/dw |A^T w|^2 = 2 A A^T w (checked against a finite difference) for the restatement itself."""
    rs = np.random.RandomState(4)
    x, w = torch.from_numpy(rs.standard_normal((2, 3, 16, 24))), torch.from_numpy(rs.standard_normal((2, 3, 16, 24)))
    G = R.affine('rot_aniso_frac', 2, 16, 24)
    C = torch.eye(4, dtype=torch.float64)[:3].expand(2, 3, 4) + 0.1 * torch.from_numpy(rs.standard_normal((2, 3, 4)))
    kw = dict(G_inv=G, C34=C, channels=(0, 3))
    ax = R.apply(x, bias=False, **kw)
    atw = R.adjoint(w, x.shape, **kw)
    assert abs(float((ax * w).sum() - (x * atw).sum())) <= 1e-10 * float(ax.abs().max() * w.abs().sum())
    g2 = R.second_order_wgrad(w, x.shape, **kw)
    d = torch.from_numpy(rs.standard_normal(tuple(w.shape)))
    eps = 1e-6
    fd = (R.adjoint(w + eps * d, x.shape, **kw).square().sum() - R.adjoint(w - eps * d, x.shape, **kw).square().sum()) / (2 * eps)
    assert abs(float(fd - (g2 * d).sum())) <= 1e-6 * abs(float(fd))


class _Pipe:
    def __init__(self, p=1.0):
        self.p = torch.tensor(p)


def test_controller_arithmetic_on_cpu_tensors():
    from shgan_amd import ada
    pipe = _Pipe(0.001)
    ctl = ada.AdaController(pipe, ada_target=0.6, ada_interval=4, ada_kimg=500)
    step = 32 * 4 / (500 * 1000)
    above = torch.tensor([1.0, 1.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0])          # mean 0.75 > 0.6
    for i in range(3):
        assert ctl.update(above, 32) == 0.0 and float(pipe.p) == pytest.approx(0.001)       # between intervals p does not move
    assert ctl.update(above, 32) == pytest.approx(step)
    assert float(pipe.p) == pytest.approx(0.001 + step, rel=1e-6) and ctl.last_mean == pytest.approx(0.75)
    below = torch.tensor([1.0, -1.0, 1.0, -1.0])                            # mean 0 < 0.6: down, floored at 0
    for i in range(8):
        ctl.update(below, 32)
    assert float(pipe.p) == pytest.approx(0.001 + step - 2 * step, abs=1e-9)
    for i in range(40):
        ctl.update(below, 32)
    assert float(pipe.p) == 0.0
    # the mean is over the interval's samples, not over its calls
    ctl2 = ada.AdaController(_Pipe(0.5), ada_target=0.0, ada_interval=2, ada_kimg=1)
    ctl2.update(torch.tensor([1.0]), 8)
    ctl2.update(torch.tensor([-1.0, -1.0, -1.0]), 8)
    assert ctl2.last_mean == pytest.approx(-0.5)


def test_pipe_refusals_and_defaults():
    from shgan_amd import ada
    for name in ('imgfilter', 'noise', 'cutout'):
        with pytest.raises(NotImplementedError, match=name):
            ada.AugmentPipe(**{name: 0.5})
    ada.AugmentPipe(imgfilter=0, noise=0, cutout=0)
    for bad in ((0, 2), (0, 4), (-1, 3), (1,)):
        with pytest.raises(ValueError):
            ada.AugmentPipe(color_channels=bad)
    with pytest.raises(ValueError):
        ada.default_color_channels(2)
    with pytest.raises(ValueError):
        ada.AugmentPipe()._color_for(2)
    with pytest.raises(ValueError):
        ada.AugmentPipe(color_channels=(2, 3))._color_for(4)              # channels 2..4 of 4
    assert ada.default_color_channels(1) == (0, 1) and ada.default_color_channels(3) == (0, 3) and ada.default_color_channels(4) == (1, 3)
    assert ada.AugmentPipe(color_channels=(0, 1))._color_for(2) == (0, 1)
    assert set(ada.AUGPIPE_SPECS) == {'blit', 'geom', 'color', 'bg', 'bgc'}
    assert len(ada.AUGPIPE_SPECS['bgc']) == 12 and all(v == 1 for v in ada.AUGPIPE_SPECS['bgc'].values())
    pipe = ada.AugmentPipe(**ada.AUGPIPE_SPECS['bgc'])
    sd = pipe.state_dict()
    assert set(sd) == {'p', 'Hz_geom'} and float(sd['p']) == 1.0 and sd['Hz_geom'].shape == (12,)
    assert abs(float(sd['Hz_geom'].double().sum()) - 1.0) < 1e-6
    assert torch.allclose(sd['Hz_geom'].double(), R.hz_geom(torch.float64), atol=1e-7)
    # defaults: everything off, ADA's strengths
    off = ada.AugmentPipe()
    assert not off.geometry_on and not off.color_on and (off.xint_max, off.scale_std, off.contrast_std, off.saturation_std) == (0.125, 0.2, 0.5, 1.0)
    with pytest.raises(Exception):
        off(torch.zeros(1, 3, 8, 8))                                       # not on the device
    from shgan_amd import losses
    with pytest.raises(NotImplementedError):
        losses.StyleGAN2Loss('cpu', None, None, None, augment_pipe=object())
