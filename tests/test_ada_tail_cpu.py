"""The tail of the ADA pipe (image-space filter, noise, cutout) without a GPU: the filter bank's closed-form properties, the restatement
(tests/ada_tail_f64.py, the yardstick of tests/test_gpu_ada_tail.py) checked against itself, and the public interface of
``ada.FullAugmentPipe``."""
import numpy as np
import pytest
import torch

import ada_tail_f64 as R


def test_filter_bank_closed_form_properties():
    fb = R.hz_fbank()
    assert fb.shape == (4, 43) and fb.dtype == np.float64
    assert np.abs(fb - fb[:, ::-1]).max() <= 1e-16                      # every row symmetric
    impulse = np.zeros(43)
    impulse[21] = 1.0
    err = np.abs(fb.sum(axis=0) - impulse).max()                        # the bands add up to the identity filter
    print(f'sum of the rows - impulse: {err:.4e}')
    # 1.0041e-12 at tap 21, a property of ADA's 16-digit sym2 constants (scipy's construction gives the same figure): the stated 1.0e-12
    # is that figure at two digits
    assert err <= 1.01e-12
    assert np.abs(fb.sum(axis=1) - np.array([1.0, 0.0, 0.0, 0.0])).max() <= 1e-15
    # the reconstruction is not exact (ADA filters a sample whose gates are all closed with this, the kernel with the impulse itself)
    assert err > 0


def test_filter_bank_per_row_convolution_is_the_two_dimensional_one():
    """ADA builds the bank with ``scipy.signal.convolve(Hz_fbank, [Hz_lo2])``, a 2-d convolution with a one-row kernel; the restatement
    convolves row by row.  Where scipy is installed the two are compared (2e-18), elsewhere the one-row 2-d convolution is spelled out."""
    lo = np.asarray(R.SYM2)
    lo2 = np.convolve(lo, lo[::-1]) / 2
    rows = np.random.RandomState(0).standard_normal((4, 13))
    per_row = np.stack([np.convolve(r, lo2) for r in rows])
    try:
        import scipy.signal
        two_d = scipy.signal.convolve(rows, [lo2])
    except ImportError:
        two_d = np.zeros((4, 19))
        for t, v in enumerate(lo2):
            two_d[:, t:t + 13] += rows * v
    assert np.abs(per_row - two_d).max() <= 1e-15
    try:                                                                # the whole bank, ADA's construction literally
        import scipy.signal
    except ImportError:
        return
    hi = lo * ((-1) ** np.arange(lo.size))
    hi2 = np.convolve(hi, hi[::-1]) / 2
    fb = np.eye(4, 1)
    for i in range(1, 4):
        fb = np.dstack([fb, np.zeros_like(fb)]).reshape(fb.shape[0], -1)[:, :-1]
        fb = scipy.signal.convolve(fb, [lo2])
        fb[i, (fb.shape[1] - hi2.size) // 2: (fb.shape[1] + hi2.size) // 2] += hi2
    err = np.abs(fb - R.hz_fbank()).max()
    print(f'bank against scipy.signal.convolve: {err:.2e}')
    assert err <= 2e-18


def test_full_pipe_interface():
    from shgan_amd import ada
    pipe = ada.FullAugmentPipe(**ada.AUGPIPE_SPECS_FULL['bgcfnc'])
    sd = pipe.state_dict()
    assert set(sd) == {'p', 'Hz_geom', 'Hz_fbank'}                       # ADA's names
    assert sd['Hz_fbank'].shape == (4, 43) and sd['Hz_fbank'].dtype == torch.float32
    assert torch.equal(sd['Hz_fbank'], torch.from_numpy(R.hz_fbank()).float())
    assert np.abs(ada.hz_fbank() - R.hz_fbank()).max() <= 1e-17
    assert isinstance(pipe, ada.AugmentPipe) and pipe.tail_on and pipe.geometry_on and pipe.color_on
    assert (pipe.imgfilter, pipe.noise, pipe.cutout) == (1.0, 1.0, 1.0)
    assert (pipe.imgfilter_bands, pipe.imgfilter_std, pipe.noise_std, pipe.cutout_size) == ((1.0, 1.0, 1.0, 1.0), 1.0, 0.1, 0.5)
    assert set(ada.AUGPIPE_SPECS) == {'blit', 'geom', 'color', 'bg', 'bgc'}
    assert set(ada.AUGPIPE_SPECS_FULL) == {'blit', 'geom', 'color', 'bg', 'bgc', 'filter', 'noise', 'cutout', 'bgcf', 'bgcfn', 'bgcfnc'}
    for key in ada.AUGPIPE_SPECS:
        assert ada.AUGPIPE_SPECS_FULL[key] == ada.AUGPIPE_SPECS[key]
    assert ada.AUGPIPE_SPECS_FULL['filter'] == dict(imgfilter=1) and ada.AUGPIPE_SPECS_FULL['noise'] == dict(noise=1)
    assert ada.AUGPIPE_SPECS_FULL['cutout'] == dict(cutout=1)
    assert ada.AUGPIPE_SPECS_FULL['bgcf'] == dict(ada.AUGPIPE_SPECS['bgc'], imgfilter=1)
    assert ada.AUGPIPE_SPECS_FULL['bgcfn'] == dict(ada.AUGPIPE_SPECS['bgc'], imgfilter=1, noise=1)
    assert ada.AUGPIPE_SPECS_FULL['bgcfnc'] == dict(ada.AUGPIPE_SPECS['bgc'], imgfilter=1, noise=1, cutout=1)
    for bands in ((1, 1, 1), (1, 1, 1, 1, 1), ()):
        with pytest.raises(ValueError, match='imgfilter_bands'):
            ada.FullAugmentPipe(imgfilter=1, imgfilter_bands=bands)
    for name in ('imgfilter', 'noise', 'cutout'):                        # the base class keeps its refusal
        with pytest.raises(NotImplementedError, match=name):
            ada.AugmentPipe(**{name: 0.5})
    off = ada.FullAugmentPipe()
    assert not off.tail_on and not off.geometry_on and not off.color_on
    tail_only = ada.FullAugmentPipe(noise=1)
    assert tail_only.tail_on and not tail_only.geometry_on
    cfg = ada.FullAugmentPipe(imgfilter=0.5, imgfilter_bands=(1, 0, 0.5, 1), noise=0.25, cutout=0.75, cutout_size=0.3)._tail_config()
    assert (cfg.imgfilter, list(cfg.bands), cfg.noise, cfg.cutout) == (0.5, [1.0, 0.0, 0.5, 1.0], 0.25, 0.75)
    assert cfg.cutout_size == pytest.approx(0.3) and cfg.noise_std == pytest.approx(0.1) and cfg.imgfilter_std == 1.0
    from shgan_amd import _lib
    with pytest.raises(_lib.ShgError, match='on the device'):
        tail_only(torch.zeros(1, 3, 32, 32))                             # not on the device
    from shgan_amd import losses
    assert losses.StyleGAN2Loss('cpu', None, None, None, augment_pipe=pipe).draw_fn == pipe.draw


def test_tail_config_matches_the_header_layout(tmp_path):
    import ctypes
    import os
    import subprocess
    from shgan_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shgan_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(shg_ada_tail_config), offsetof(shg_ada_tail_config, bands), '
                   'offsetof(shg_ada_tail_config, imgfilter_std), offsetof(shg_ada_tail_config, noise_std), '
                   'offsetof(shg_ada_tail_config, cutout_size)); return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)])
    T = _lib.AdaTailConfig
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [ctypes.sizeof(T), T.bands.offset, T.imgfilter_std.offset,
                                                                             T.noise_std.offset, T.cutout_size.offset]


def _case(seed, shape):
    rs = np.random.RandomState(seed)
    N = shape[0]
    ut, gt = torch.from_numpy(rs.uniform(size=(N, 8))), torch.from_numpy(rs.standard_normal((N, 5)))
    x, w = torch.from_numpy(rs.standard_normal(shape)), torch.from_numpy(rs.standard_normal(shape))
    return ut, gt, x, w


def test_restatement_adjoint_and_second_order_are_consistent():
    """<A x, w> = <x, A^T w> for the restatement's linear part, which is not self-adjoint (the reflected pad folds back), and
    d/dw |A^T w|^2 = 2 A A^T w against A applied to A^T w."""
    shape = (2, 4, 22, 26)
    ut, gt, x, w = _case(1, shape)
    pr = R.params(ut, gt, 1.0, dict(imgfilter=1, cutout=1), torch.float64)
    assert bool(pr['fired'].all())
    kw = dict(Hz=pr['Hz'], cut=pr['cut'], channels=(1, 3))
    ax = R.apply(x, bias=False, **kw)
    atw = R.adjoint(w, **kw)
    lhs, rhs = float((ax * w).sum()), float((x * atw).sum())
    assert abs(lhs - rhs) <= 1e-10 * float(ax.abs().max() * w.abs().sum())
    aw = R.apply(w, bias=False, **kw)
    gap = float((atw - aw).abs().max())
    print(f'max |A^T w - A w| = {gap:.3f}')
    assert gap > 1e-2
    g2 = R.second_order_wgrad(w, **kw)
    assert float((g2 - 2 * R.apply(atw, bias=False, **kw)).abs().max()) <= 1e-10 * float(g2.abs().max())


def test_restatement_with_all_gates_closed_returns_its_input():
    shape = (3, 3, 24, 40)
    ut, gt, x, _ = _case(2, shape)
    cfg = dict(imgfilter=1, noise=1, cutout=1)
    pr = R.params(ut, gt, 0.0, cfg, torch.float64)
    assert not bool(pr['fired'].any()) and float(pr['sigma'].abs().max()) == 0.0 and float(pr['cut'][:, 2:].abs().max()) == 0.0
    z = torch.from_numpy(np.random.RandomState(3).standard_normal(shape))
    y = R.apply(x, Hz=pr['Hz'], sigma=pr['sigma'], z=z, cut=pr['cut'], channels=(0, 3))
    err = float((y - x).abs().max())
    print(f'all gates closed: max |y - x| = {err:.2e}')
    assert err <= 1e-11
    open_ = R.params(ut, gt, 1.0, cfg, torch.float64)
    y1 = R.apply(x, Hz=open_['Hz'], sigma=open_['sigma'], z=z, cut=open_['cut'], channels=(0, 3))
    assert float((y1 - x).abs().max()) > 1e-2 and int((y1 == 0).sum()) > 0


def test_restatement_gains_follow_the_expected_power_normalisation():
    """One band alone: g = t / sqrt(sum(expected_power t^2)) with t_i in place i, the others 1; Hz' = g @ bank."""
    ut = torch.full((1, 8), 0.5, dtype=torch.float64)
    gt = torch.tensor([[0.0, 1.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    pr = R.params(ut, gt, 1.0, dict(imgfilter=1, imgfilter_bands=(0, 1, 0, 0)), torch.float64)
    assert pr['fired'].tolist() == [[False, True, False, False]]
    t = np.array([1.0, 2.0, 1.0, 1.0])
    g = t / np.sqrt((np.array([10, 1, 1, 1]) / 13 * t * t).sum())
    assert np.abs(pr['Hz'].numpy()[0] - g @ R.hz_fbank()).max() <= 1e-15
