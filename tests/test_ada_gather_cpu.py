"""The gather-form ADA adjoint without a GPU: the factorisation P^T U^T S^T D^T C^T (tests/ada_gather_f64.py) against autograd of the literal
restatement, the candidate window of csrc/ada_geom.h proved by brute force in a host build, what the two new entry points of the C ABI
refuse, and the ``deterministic`` keyword of the public interface."""
import ctypes
import inspect
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import shgan_amd  # noqa: F401
from shgan_amd import _lib, ada

import ada_f64 as R
import ada_gather_f64 as RG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sh-gan_amd', 'csrc')
NEW = ('shg_ada_adjoint_gather_workspace_bytes', 'shg_ada_apply_adjoint_gather_f32')
SMALL = [(3, 1, 16, 16), (2, 3, 16, 24), (2, 4, 24, 16)]
CH = {1: (0, 1), 3: (0, 3), 4: (1, 3)}


def margins_of(G, H, W):
    return tuple(int(v) for v in R.margins_pre(G.double(), H, W).ceil())


# ---- the factorisation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.AFFINE_KINDS)
@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_factorisation_equals_autograd_of_the_restatement(shape, kind):
    """P^T U^T S^T D^T C^T in float64 against ``ada_f64.adjoint`` (autograd through F.pad, the two FIR passes and grid_sample): 1e-12 of the
    largest value.  This pins o - 2 i + 5, the parity rule of the decimation and the three reflect preimages."""
    N, C, H, W = shape
    rs = np.random.RandomState(sum(shape) + len(kind))
    w = torch.from_numpy(rs.standard_normal(shape))
    G = R.affine(kind, N, H, W).float().double()
    Cm = torch.eye(4, dtype=torch.float64)[:3].expand(N, 3, 4) + 0.1 * torch.from_numpy(rs.standard_normal((N, 3, 4)))
    m = margins_of(G, H, W)
    want = R.adjoint(w, shape, G_inv=G, C34=Cm, channels=CH[C], margins=m)
    got = RG.adjoint(w, G_inv=G, C34=Cm, channels=CH[C], margins=m)
    err = float((got - want).abs().max()) / max(float(want.abs().max()), 1.0)
    print(f'factorisation {shape} {kind}: {err:.2e}')
    assert err <= 1e-12
    geo = float((RG.adjoint(w, G_inv=G, margins=m) - R.adjoint(w, shape, G_inv=G, margins=m)).abs().max())
    col = float((RG.adjoint(w, C34=Cm, channels=CH[C]) - R.adjoint(w, shape, C34=Cm, channels=CH[C])).abs().max())
    assert geo <= 1e-12 * max(float(want.abs().max()), 1.0) and col <= 1e-12 * max(float(want.abs().max()), 1.0)


# ---- the window ---------------------------------------------------------------------------------------------------------------------------
def routing_matrices():
    """Matrices the gather route must leave to the scatter kernel: beyond ADA_GATHER_HMAX, singular, not finite, beyond ADA_GATHER_MAG."""
    far = R.scale2d(1 / 64, 1 / 64, torch.float64)
    singular = torch.tensor([[1.0, 2.0, 0.5], [0.5, 1.0, -0.25], [0.0, 0.0, 1.0]], dtype=torch.float64)
    nan = torch.eye(3, dtype=torch.float64)
    nan[0, 1] = float('nan')
    inf = torch.eye(3, dtype=torch.float64)
    inf[1, 2] = float('inf')
    huge = R.translate2d(3e7, 0.0, torch.float64)
    steep = R.scale2d(1e6, 1e6, torch.float64)
    return dict(far=far, singular=singular, nan=nan, inf=inf, huge=huge, steep=steep)


def _window_cases():
    cases = []                                             # (label, H, W, margins, G [3,3] float32, the gather takes it)
    for H, W in ((16, 24), (40, 72)):
        for kind in R.AFFINE_KINDS:
            Gs = R.affine(kind, 2, H, W).float()
            m = margins_of(Gs, H, W)
            for n in range(2):
                cases.append((f'{kind}[{n}]', H, W, m, Gs[n], True))
        for name, G in routing_matrices().items():
            cases.append((name, H, W, (6, 6, 6, 6), G.float(), False))
        rs = np.random.RandomState(H + W)
        for k in range(150):                                # rotation x anisotropy x isotropic scale x shift, ADA's ranges and beyond
            th0, th1 = rs.uniform(-math.pi, math.pi, size=2)
            s, a = 2.0 ** rs.uniform(-2.0, 2.0), 2.0 ** rs.uniform(-1.0, 1.0)
            G = (R.rotate2d_inv(-th0, torch.float64) @ R.scale2d_inv(s * a, s / a, torch.float64) @ R.rotate2d_inv(-th1, torch.float64)
                 @ R.translate2d_inv(rs.uniform(-0.3, 0.3) * W, rs.uniform(-0.3, 0.3) * H, torch.float64)).float()
            cases.append((f'random{k}', H, W, margins_of(G[None], H, W), G, True))
    return cases


def test_candidate_window_holds_every_touching_sample(tmp_path):
    """csrc/ada_geom.h compiled as host C++ (tests/ada_gather_window_check.cpp): for every named matrix of the device tests and 150 random
    rotation x scale x anisotropy x shift matrices per size, at 16 x 24 and 40 x 72, every sample whose floor(c) or floor(c) + 1 equals an
    upsampled pixel v lies inside v's candidate window; the routing matrices are refused; no window exceeds (2 * 24 + 1)^2 candidates."""
    exe = tmp_path / 'window_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-Wno-unused-function', '-Wno-unknown-pragmas', '-I', CSRC,
                           os.path.join(ROOT, 'tests', 'ada_gather_window_check.cpp'), '-o', str(exe)])
    cases = _window_cases()
    text = ''.join(f'{H} {W} {m[0]} {m[1]} {m[2]} {m[3]} ' + ' '.join(float(v).hex() if math.isfinite(float(v)) else str(float(v)) for v in G[:2].reshape(-1))
                   + '\n' for _, H, W, m, G, _ in cases)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split('\n')
    rows = [[int(v) for v in line.split()] for line in out if line.strip()]
    assert len(rows) == len(cases)
    worst = 0
    for (label, H, W, m, G, takes), (ok, touched, bad, largest) in zip(cases, rows):
        assert bool(ok) == takes, (label, H, W, ok)
        if takes:
            assert touched > 0 and bad == 0, (label, H, W, touched, bad)
            assert largest <= 49 * 49, (label, largest)
            worst = max(worst, largest)
    print(f'{len(cases)} matrices, largest candidate window {worst}')


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name + '(' in hdr and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert _lib.get_lib().shg_abi_version() == _lib.ABI_VERSION == 40


def test_entry_points_refuse_bad_arguments():
    lib = _lib.get_lib()
    p = ctypes.c_void_p
    N, C, H, W = 2, 3, 16, 24
    need = lib.shg_ada_adjoint_gather_workspace_bytes(N, C, H, W)
    assert need == N * C * (2 * H + 10) * (2 * W + 10) * 4
    for bad in ((0, C, H, W), (N, 0, H, W), (N, C, 0, W), (N, C, H, 16385), (65536, 1, H, W)):
        assert lib.shg_ada_adjoint_gather_workspace_bytes(*bad) == 0, bad
    f = lib.shg_ada_apply_adjoint_gather_f32

    def refused(*args, word):
        rc = f(*args)
        msg = lib.shg_last_error()
        assert rc == -1 and b'ada_apply_adjoint_gather_f32' in msg and word in msg, (rc, msg)
    gy, G, Cm, mg, gx, ws = p(64), p(128), p(192), p(256), p(320), p(384)         # never dereferenced: every call below is refused on the host
    refused(None, G, Cm, mg, gx, ws, need, N, C, H, W, 1, 0, 3, None, word=b'null')
    refused(gy, G, Cm, mg, None, ws, need, N, C, H, W, 1, 0, 3, None, word=b'null')
    refused(gy, G, Cm, mg, gy, ws, need, N, C, H, W, 1, 0, 3, None, word=b'aliased')
    refused(gy, G, Cm, mg, gx, ws, need, 0, C, H, W, 1, 0, 3, None, word=b'>= 1')
    refused(gy, G, Cm, mg, gx, ws, need, N, C, H, 16385, 1, 0, 3, None, word=b'16384')
    refused(gy, G, Cm, mg, gx, ws, need, N, C, H, W, 2, 0, 3, None, word=b'geom')
    refused(gy, G, Cm, mg, gx, ws, need, N, C, H, W, 1, 0, 2, None, word=b'color_count')
    refused(gy, G, Cm, mg, gx, ws, need, N, C, H, W, 1, 1, 3, None, word=b'outside')
    refused(gy, G, Cm, mg, gx, ws, need, N, C, H, W, 0, 0, 0, None, word=b'nothing to do')
    refused(gy, None, Cm, mg, gx, ws, need, N, C, H, W, 1, 0, 3, None, word=b'geometry needs')
    refused(gy, G, Cm, None, gx, ws, need, N, C, H, W, 1, 0, 3, None, word=b'geometry needs')
    refused(gy, G, None, mg, gx, ws, need, N, C, H, W, 1, 0, 3, None, word=b'colour needs')
    refused(gy, G, Cm, mg, gx, None, need, N, C, H, W, 1, 0, 3, None, word=b'workspace')
    refused(gy, G, Cm, mg, gx, ws, need - 1, N, C, H, W, 1, 0, 3, None, word=b'workspace')
    refused(gy, G, Cm, mg, gx, ws, 0, N, C, H, W, 1, 0, 0, None, word=b'workspace')
    refused(gy, G, Cm, mg, gx, gx, need, N, C, H, W, 1, 0, 3, None, word=b'aliases')


# ---- the public interface -------------------------------------------------------------------------------------------------------------------
def test_deterministic_keyword_is_off_by_default_and_not_state():
    for fn in (ada.ada_apply, ada.ada_apply_adjoint, ada.AugmentPipe.__init__, ada.FullAugmentPipe.__init__):
        assert inspect.signature(fn).parameters['deterministic'].default is False, fn
    for cls, spec in ((ada.AugmentPipe, ada.AUGPIPE_SPECS['bgc']), (ada.FullAugmentPipe, ada.AUGPIPE_SPECS_FULL['bgcfnc'])):
        off, on = cls(**spec), cls(**spec, deterministic=True)
        assert off.deterministic is False and on.deterministic is True
        assert sorted(on.state_dict()) == sorted(off.state_dict()) and not any('deterministic' in k for k in on.state_dict())
        off.load_state_dict(on.state_dict())
        assert off.deterministic is False
    x = torch.zeros(1, 3, 16, 16)
    assert ada.ada_apply_adjoint(x, deterministic=True) is x                    # nothing to do: the tensor itself, as without the keyword
    with pytest.raises(_lib.ShgError):                                             # no CPU route behind the keyword either
        ada.ada_apply_adjoint(x, G_inv=torch.eye(3).reshape(1, 3, 3), margins=torch.tensor([6, 6, 6, 6], dtype=torch.int32), deterministic=True)
