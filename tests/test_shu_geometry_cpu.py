"""CPU (no GPU): host side of the size-general Spectral Hint Unit -- constant tables against the reference's at the geometries of
tests/golden/shu_geometry*.npz (tools/gen_golden_shu_geometry.py), the constructor's supported set and its rejections, the ``shu=``
override of ``configs.model_cfg``, and the argument checks of the ``shg_shu_*_n_f32`` entry points (host code)."""
import ctypes

import numpy as np
import pytest

import shgan_amd  # noqa: F401
from conftest import load_golden
from shgan_amd import _lib, configs
from shgan_amd.model_zoo import shgan

CASE_FILES = {'A': 'shu_geometry', 'B': 'shu_geometry_128', 'C': 'shu_geometry', 'D': 'shu_geometry', 'E': 'shu_geometry_128'}


def build_case(cid):
    """-> (SHU of case ``cid`` with the fixture's parameters, fixture file, (batch, channels, size, lowest, seed))."""
    import torch
    g = load_golden(CASE_FILES[cid])
    n, c, size, lowest, gtop, fh, fw, seed = [int(v) for v in g[f'{cid}__cfg']]
    shu = shgan.SHU(c, c, [fh, fw], str(g[f'{cid}__type']), input_res=size, lowest_res=lowest, tail_sigma_mult=3,
                    gaussian_at_input_res=bool(gtop))
    shu.load_state_dict({k: torch.from_numpy(g[f'{cid}__sd__{k}']) for k in ('conv0.weight', 'conv0.bias', 'df1.weight')}, strict=True)
    return shu, g, (n, c, size, lowest, seed)


@pytest.mark.parametrize('cid', sorted(CASE_FILES))
def test_tables_match_the_reference(cid):
    shu, _, (_, _, size, lowest, _) = build_case(cid)
    tab = load_golden('shu_geometry_tables')
    res = [r for r in (4, 8, 16, 32, 64, 128) if lowest <= r <= size]
    assert shu.reslist == res
    for r in res:
        assert np.abs(shu.gaussian_weight_map[r].numpy() - tab[f'{cid}__gauss{r}']).max() < 1e-7, r
        assert np.array_equal(getattr(shu, f'_gauss{r}').numpy(), shu.gaussian_weight_map[r].numpy())
    assert tuple(shu._cw.shape) == tuple(tab[f'{cid}__cw'].shape)
    assert np.abs(shu._cw.numpy() - tab[f'{cid}__cw']).max() < 1e-7
    assert '_cw' not in shu.state_dict()


def test_constructor_supported_set_and_rejections():
    for size in (16, 32, 64, 128):
        lowest = 4
        while lowest <= size:
            for gtop in (False, True):
                assert shgan.SHU(8, 8, [2, 3], 'piecewise_linear', size, lowest, gaussian_at_input_res=gtop).reslist[-1] == size
            lowest *= 2
    with pytest.raises(NotImplementedError, match='LDS'):
        shgan.SHU(32, 32, [2, 3], 'piecewise_linear', input_res=256, lowest_res=4)
    with pytest.raises(NotImplementedError, match='LDS'):
        shgan.SHU(32, 32)                                                  # the reference's default input_res
    with pytest.raises(NotImplementedError, match='16, 32, 64, 128'):
        shgan.SHU(32, 32, [2, 3], 'piecewise_linear', input_res=8, lowest_res=4)
    with pytest.raises(NotImplementedError, match='powers of two'):
        shgan.SHU(32, 32, [2, 3], 'piecewise_linear', input_res=48, lowest_res=4)
    with pytest.raises(NotImplementedError, match='in_channels 32 != out_channels 16'):
        shgan.SHU(32, 16, [2, 3], 'piecewise_linear', input_res=64, lowest_res=4)
    for lowest in (2, 12, 128):
        with pytest.raises(NotImplementedError, match='lowest_res'):
            shgan.SHU(32, 32, [2, 3], 'piecewise_linear', input_res=64, lowest_res=lowest)


def test_model_cfg_shu_override_round_trips():
    base = configs.model_cfg('shgan_g256')
    assert configs.model_cfg('shgan_g256', shu=None) == base and configs.model_cfg('shgan_g256', shu={}) == base
    over = dict(shu_input_res=32, shu_lowest_res=8, shu_channels=16, shu_gaussian_at_input_res=True)
    cfg = configs.model_cfg('shgan_g256', shu=over)
    enc = cfg['args']['encoder']['args']
    assert all(enc[k] == v for k, v in over.items())
    assert set(enc) == set(base['args']['encoder']['args'])
    assert {k: v for k, v in enc.items() if k not in over} == {k: v for k, v in base['args']['encoder']['args'].items() if k not in over}
    assert set(configs.SHU_KEYS) == {k for k in enc if k.startswith('shu_')}
    with pytest.raises(KeyError, match='shu_res'):
        configs.model_cfg('shgan_g256', shu=dict(shu_res=32))
    G = configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128, shu=dict(shu_input_res=32, shu_lowest_res=8))
    assert G.encoder.shu.reslist == [8, 16, 32] and G.encoder.shu.input_res == 32
    ref = configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128)
    assert {k: tuple(v.shape) for k, v in G.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    with pytest.raises(NotImplementedError, match='LDS'):
        configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128, shu=dict(shu_input_res=256))


def test_abi_version_and_shipped_symbols_stay():
    lib = _lib.get_lib()
    assert lib.shg_abi_version() == 40 == _lib.ABI_VERSION          # symbols were added, nothing changed
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('shg_shu_rfft2_shift_f32', 'shg_shu_spectral_f32', 'shg_shu_split_irfft2_f32', 'shg_shu_split_adjoint_f32',
                 'shg_shu_rfft2_shift_n_f32', 'shg_shu_spectral_n_f32', 'shg_shu_split_irfft2_n_f32', 'shg_shu_split_adjoint_n_f32'):
        assert hasattr(raw, name), name
    # the shipped entry points keep their checks
    P = ctypes.c_void_p(16)
    assert lib.shg_shu_spectral_f32(P, P, P, P, P, P, 1, 64, 544, 6, None) == -1 and b'P % 64' in lib.shg_last_error()


def test_size_general_entry_points_validate_their_arguments_without_a_gpu():
    lib = _lib.get_lib()
    P = ctypes.c_void_p(16)

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def ptrs(*v):
        return (ctypes.c_void_p * len(v))(*v)

    def longs(*v):
        return (ctypes.c_long * len(v))(*v)

    f = lib.shg_shu_rfft2_shift_n_f32
    assert f(None, 0, P, 1, 4, 32, None) == -1 and b'null' in lib.shg_last_error()
    for bad in (8, 48, 256, 0, -64):
        assert f(P, 0, P, 1, 4, bad, None) == -1 and b'16, 32, 64 or 128' in lib.shg_last_error() and str(bad).encode() in lib.shg_last_error()
    assert b'LDS' in lib.shg_last_error()
    assert f(P, 0, P, 0, 4, 32, None) == -1 and b'shape' in lib.shg_last_error()

    f = lib.shg_shu_spectral_n_f32
    assert f(P, P, None, P, P, P, 1, 64, 544, 6, None) == -1 and b'null' in lib.shg_last_error()
    assert f(P, P, P, P, P, P, 1, 32, 544, 6, None) == -1 and b'64 spectral channels' in lib.shg_last_error()
    assert f(P, P, P, P, P, P, 1, 64, 546, 6, None) == -1 and b'P % 4' in lib.shg_last_error()
    assert f(P, P, P, P, P, P, 1, 64, 544, 9, None) == -1 and b'8 bands' in lib.shg_last_error()
    assert f(ctypes.c_void_p(8), P, P, P, P, P, 1, 64, 544, 6, None) == -1 and b'aligned' in lib.shg_last_error()

    f = lib.shg_shu_split_irfft2_n_f32
    g3, o3, s3 = ptrs(16, 16, 16), ptrs(16, 16, 16), longs(0, 0, 0)
    assert f(None, None, g3, o3, s3, 1, 4, 1, 0, 32, ints(8, 16, 32), 3, None) == -1 and b'null' in lib.shg_last_error()
    assert f(P, None, g3, o3, s3, 1, 4, 1, 0, 32, None, 3, None) == -1 and b'null' in lib.shg_last_error()
    assert f(P, None, g3, o3, s3, 1, 4, 1, 0, 256, ints(64, 128, 256), 3, None) == -1 and b'16, 32, 64 or 128' in lib.shg_last_error()
    for res in ((8, 16, 64), (4, 8, 16), (16, 16, 32), (32, 16, 8), (2, 4, 32)):
        assert f(P, None, g3, o3, s3, 1, 4, 1, 0, 32, ints(*res), 3, None) == -1 and b'consecutive powers of two' in lib.shg_last_error(), res
    assert f(P, None, g3, o3, s3, 1, 4, 1, 0, 32, ints(8, 16, 32), 0, None) == -1 and b'consecutive powers of two' in lib.shg_last_error()
    assert f(P, None, g3, o3, s3, 1, 4, 1, 0, 16, ints(2, 4, 8, 16), 4, None) == -1 and b'consecutive powers of two' in lib.shg_last_error()
    assert f(P, None, g3, o3, s3, 1, 4, 6, 0, 32, ints(8, 16, 32), 3, None) == -1 and b'cw required' in lib.shg_last_error()
    assert f(P, None, ptrs(16, None, 16), o3, s3, 1, 4, 1, 0, 32, ints(8, 16, 32), 3, None) == -1 and b'table for level 1' in lib.shg_last_error()
    assert f(P, None, g3, o3, s3, 1, 0, 1, 0, 32, ints(8, 16, 32), 3, None) == -1 and b'shape' in lib.shg_last_error()

    f = lib.shg_shu_split_adjoint_n_f32
    assert f(g3, s3, g3, None, 1, 4, 32, ints(8, 16, 32), 3, None) == -1 and b'null' in lib.shg_last_error()
    assert f(g3, s3, g3, P, 1, 4, 48, ints(12, 24, 48), 3, None) == -1 and b'16, 32, 64 or 128' in lib.shg_last_error()
    assert f(g3, s3, g3, P, 1, 4, 128, ints(8, 16, 32), 3, None) == -1 and b'consecutive powers of two' in lib.shg_last_error()
    assert f(g3, s3, ptrs(16, 16, None), P, 1, 4, 32, ints(8, 16, 32), 3, None) == -1 and b'table for level 2' in lib.shg_last_error()
    assert f(g3, s3, g3, P, 70000, 4, 32, ints(8, 16, 32), 3, None) == -1 and b'shape' in lib.shg_last_error()


def test_python_wrappers_reject_what_the_kernels_do_not_take():
    import torch
    from shgan_amd import kernels
    with pytest.raises(_lib.ShgError, match='HIP tensor'):
        kernels.shu_rfft2_shift(torch.zeros(1, 2, 32, 32))                 # a CPU tensor: no fallback
    with pytest.raises(_lib.ShgError, match='transform size'):
        kernels._shu_levels(256, 3, 'test')
    with pytest.raises(_lib.ShgError, match='levels'):
        kernels._shu_levels(16, 4, 'test')
    assert kernels._shu_levels(64, 5, 'test') == ([4, 8, 16, 32, 64], None)          # the shipped geometry: the fixed entry points
    res, arr = kernels._shu_levels(128, 2, 'test')
    assert res == [64, 128] and list(arr) == [64, 128]
