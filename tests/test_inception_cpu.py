"""CPU (no GPU): the FID detector's host side -- state_dict validation, BatchNorm folding, the TF1 front-end mapping, the C ABI's
argument checks and export list (sh-gan_amd/inception.py, csrc/inception.hip), and EvalLoop's real-side FID bookkeeping."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import shgan_amd  # noqa: F401
from conftest import ROOT
from shgan_amd import _lib, inception

import inception_f64 as ref

NEW = ('shg_inception_frontend_f32', 'shg_inception_packed_weight_elems', 'shg_inception_weight_prep_f32', 'shg_inception_conv_workspace_bytes',
       'shg_inception_conv_f32', 'shg_inception_pool_f32', 'shg_inception_mean_f32')


def _sd_meta():
    return {k: torch.empty(0).new_zeros(s) for k, s in inception.expected_shapes().items()}


def test_layer_table_matches_the_float64_model_and_counts_94_convolutions():
    assert len(inception.LAYERS) == 94
    assert [(n, i, o, k) for n, (i, o, k, _, _, _) in inception.LAYERS.items()] == ref.TABLE
    sd = ref.random_state_dict(0)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(inception.expected_shapes())
    macs = inception.macs_per_image()
    assert 5.6e9 < macs < 5.8e9, macs


def test_state_dict_validation_names_the_key():
    sd = _sd_meta()
    inception.validate_state_dict(sd)
    ok = dict(sd, **{'fc.weight': torch.zeros(1008, 2048), 'fc.bias': torch.zeros(1008), 'AuxLogits.fc.weight': torch.zeros(3),
                     'Mixed_6b.branch1x1.bn.num_batches_tracked': torch.zeros((), dtype=torch.long)})
    inception.validate_state_dict(ok)                   # classifier / auxiliary head ignored, BN step counter accepted
    miss = dict(sd)
    del miss['Mixed_6c.branch7x7dbl_3.bn.running_var']
    with pytest.raises(_lib.ShgError, match=r"Mixed_6c\.branch7x7dbl_3\.bn\.running_var"):
        inception.validate_state_dict(miss)
    extra = dict(sd, **{'Mixed_5b.branch9x9.conv.weight': torch.zeros(1)})
    with pytest.raises(_lib.ShgError, match=r"Mixed_5b\.branch9x9\.conv\.weight"):
        inception.validate_state_dict(extra)
    bad = dict(sd, **{'Mixed_7c.branch3x3_2b.conv.weight': torch.zeros(384, 384, 1, 3)})
    with pytest.raises(_lib.ShgError, match=r"Mixed_7c\.branch3x3_2b\.conv\.weight.*\(384, 384, 1, 3\)"):
        inception.validate_state_dict(bad)
    with pytest.raises(_lib.ShgError, match=r"Conv2d_1a_3x3\.conv\.weight"):
        inception.InceptionFeatures.from_state_dict({k: v for k, v in sd.items() if k != 'Conv2d_1a_3x3.conv.weight'}, device='cpu')


def test_bn_folding_in_float64_equals_conv_then_bn():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(48, 32, 1, 7, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(48, generator=g, dtype=torch.float64) + 0.5, torch.randn(48, generator=g, dtype=torch.float64)
    mean, var = torch.randn(48, generator=g, dtype=torch.float64), torch.rand(48, generator=g, dtype=torch.float64) + 0.1
    x = torch.randn(2, 32, 11, 13, generator=g, dtype=torch.float64)
    want = F.batch_norm(F.conv2d(x, w, padding=(0, 3)), mean, var, gamma, beta, training=False, eps=1e-3)
    wf, bf = inception.fold_bn(w.float(), gamma.float(), beta.float(), mean.float(), var.float())
    assert wf.dtype == torch.float64 and bf.shape == (48,)
    wf64, bf64 = inception.fold_bn(w, gamma, beta, mean, var)
    got = F.conv2d(x, wf64, bf64, padding=(0, 3))
    assert float((got - want).abs().max() / want.abs().max()) < 1e-14


@pytest.mark.parametrize('size', [256, 512, 1024, 299, (200, 300)])
def test_tf1_resize_formula_equals_the_affine_grid_form(size):
    """Source coordinate i * W / 299, no half-pixel offset, border clamp == affine_grid(shifted theta) + grid_sample(bilinear, border,
    align_corners=False), in float64."""
    h, w = (size, size) if isinstance(size, int) else size
    x = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(h), dtype=torch.float64) * 255
    a, b = ref.resize_tf1(x), ref.resize_grid(x)
    assert a.shape == b.shape == (2, 3, 299, 299)
    assert float((a - b).abs().max()) < 1e-9
    if h == w == 299:
        assert float((a - x).abs().max()) < 1e-9        # the identity: the product skips the resize there


def test_value_maps_follow_the_reference():
    u8 = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 16, 16).repeat(1, 3, 1, 1)
    assert torch.equal(ref.values_f32(u8), u8.float())
    real = u8.float().div(255) * 2 - 1
    assert torch.equal(ref.values_f32(u8, 'pm1'), real * 127.5 + 127.5)
    assert torch.equal(ref.values_f32(real, 'pm1'), real * 127.5 + 127.5)
    from shgan_amd import kernels
    assert torch.equal(kernels.u8_value_table('cpu') * 127.5 + 127.5, ref.values_f32(torch.arange(256, dtype=torch.uint8), 'pm1'))


def _desc(**kw):
    d = dict(x=16, w=16, bias=16, y=16, I=64, H=17, W=17, x_ctot=64, x_coff=0, O=96, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, OH=17, OW=17,
             y_ctot=96, y_coff=0, splitk=1)
    d.update(kw)
    return _lib.IncConv(**d)


def _conv_rc(descs, B=2, ws=None, nbytes=0):
    arr = (_lib.IncConv * len(descs))(*descs)
    return _lib.get_lib().shg_inception_conv_f32(arr, len(descs), B, ws, nbytes, None)


def test_abi_argument_checks_reject_bad_calls_without_a_gpu():
    lib = _lib.get_lib()
    err = lambda: lib.shg_last_error().decode()        # noqa: E731
    assert _conv_rc([_desc(y=None)]) == -1 and 'null' in err()
    assert lib.shg_inception_conv_f32(None, 1, 2, None, 0, None) == -1
    assert _conv_rc([_desc()] * 9) == -1                                      # more than SHG_INC_MAX_GROUPS
    assert _conv_rc([_desc()], B=0) == -1
    assert _conv_rc([_desc(OH=16)]) == -1 and 'geometry' in err()
    assert _conv_rc([_desc(kh=9, ph=1)]) == -1 and 'not supported' in err()
    assert _conv_rc([_desc(sh=3)]) == -1
    assert _conv_rc([_desc(ph=3)]) == -1                                      # pad >= kernel
    assert _conv_rc([_desc(y_ctot=2048, y_coff=1953)]) == -1 and 'offset 1953' in err()
    assert _conv_rc([_desc(x_ctot=64, x_coff=1)]) == -1 and 'input' in err()
    assert _conv_rc([_desc(w=8)]) == -1 and 'aligned' in err()
    assert _conv_rc([_desc(splitk=17)]) == -1
    assert _conv_rc([_desc(I=16, kh=1, kw=1, ph=0, pw=0, splitk=2)]) == -1 and 'split' in err()   # one K step cannot be split in two
    # workspace: the query sums splitk * O * pixels floats over the splitting groups; a smaller one is refused before any launch
    descs = [_desc(), _desc(splitk=4, I=448, x_ctot=448, y_ctot=384, O=384)]
    arr = (_lib.IncConv * 2)(*descs)
    need = lib.shg_inception_conv_workspace_bytes(arr, 2, 2)
    assert need == 4 * 384 * 2 * 17 * 17 * 4
    assert _conv_rc(descs, ws=None, nbytes=0) == -1 and 'workspace' in err()
    assert _conv_rc(descs, ws=ctypes.c_void_p(16), nbytes=need - 4) == -1 and 'too small' in err()
    assert lib.shg_inception_conv_workspace_bytes(arr, 1, 2) == 0
    assert lib.shg_inception_packed_weight_elems(48, 192, 1, 1) == 192 * 64
    assert lib.shg_inception_packed_weight_elems(32, 3, 3, 3) == 32 * 64
    assert lib.shg_inception_packed_weight_elems(0, 3, 3, 3) == -1
    p = ctypes.c_void_p(16)
    assert lib.shg_inception_weight_prep_f32(None, p, p, p, 32, 3, 3, 3, None) == -1
    assert lib.shg_inception_weight_prep_f32(p, p, p, p, 32, 3, 9, 3, None) == -1
    assert lib.shg_inception_frontend_f32(None, None, 1.0, 0.0, p, 1, 8, 8, None) == -1
    assert lib.shg_inception_frontend_f32(p, None, 1.0, 0.0, p, 0, 8, 8, None) == -1
    assert lib.shg_inception_pool_f32(p, None, 1, 8, 8, 8, 0, 1, 1, 8, 0, None) == -1
    assert lib.shg_inception_pool_f32(p, p, 1, 8, 8, 8, 2, 1, 1, 8, 0, None) == -1
    assert lib.shg_inception_pool_f32(p, p, 1, 8, 8, 8, 0, 1, 1, 10, 3, None) == -1 and 'offset' in err()
    assert lib.shg_inception_mean_f32(p, None, 1, 8, 64, None) == -1
    assert lib.shg_inception_mean_f32(p, p, 1, 8, 0, None) == -1


def test_exports_signatures_and_descriptor_layout(tmp_path):
    hdr = open(os.path.join(ROOT, 'include', 'shgan_hip.h')).read()
    declared = set(re.findall(r'\b(shg_[a-z0-9_]+)\s*\(', hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.exported_symbols() and hasattr(lib, name)
    assert _lib.ABI_VERSION == 40 and _lib.get_lib().shg_abi_version() == 40
    assert _lib._SIGS['shg_inception_conv_f32'][0] == ctypes.POINTER(_lib.IncConv)
    assert _lib.get_lib().shg_inception_conv_workspace_bytes.restype == ctypes.c_size_t
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shgan_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(shg_inc_conv_desc), offsetof(shg_inc_conv_desc, y), '
                   'offsetof(shg_inc_conv_desc, I), offsetof(shg_inc_conv_desc, O), offsetof(shg_inc_conv_desc, splitk), SHG_INC_MAX_GROUPS); '
                   'return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    D = _lib.IncConv
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [ctypes.sizeof(D), D.y.offset, D.I.offset, D.O.offset,
                                                                            D.splitk.offset, inception.MAX_GROUPS]


def test_host_tensors_are_refused():
    with pytest.raises(_lib.ShgError):
        inception.frontend(torch.zeros(1, 3, 8, 8))
    with pytest.raises(_lib.ShgError):
        inception.frontend(torch.zeros(1, 3, 8, 8), input_range='01')


def test_eval_loop_real_side_moments_on_the_cpu():
    """fid_real=True: the loop runs feature_fn on each batch's real (input_range='pm1') into per-stream partials of their own, padded
    duplicates weigh 0; gather() reduces both sides; fid_value() = fid_from_stats on them.  Stand-ins for G and the detector."""
    from shgan_amd import eval_harness as hz
    from shgan_amd.fid_stats import fid_from_stats
    R, N, D = 8, 7, 6
    calls = []

    def feat(img, input_range='0_255'):
        calls.append(input_range)
        v = img.to(torch.float64)
        if input_range == 'pm1':
            v = v * 127.5 + 127.5
        return v.reshape(img.shape[0], -1)[:, :D].to(torch.float32)

    def acc(S, f, w):
        f = f.to(torch.float64)
        w = torch.ones(f.shape[0], dtype=torch.float64) if w is None else w.to(torch.float64)
        x = torch.cat([f, torch.ones(f.shape[0], 1, dtype=torch.float64)], 1)
        S[:D + 1, :D + 1] += (x * w[:, None]).T @ x

    def step(x4, z, out):
        img = ((x4[:, 1:] + 1) * 100).clamp(0, 255).to(torch.uint8)
        if out is not None:
            out.copy_(img)
        return img

    class Loader:
        def __init__(self, ids):
            self.ids = ids

        def __iter__(self):
            for b0 in range(0, len(self.ids), 3):
                ids = self.ids[b0:b0 + 3]
                g = torch.Generator().manual_seed(b0)
                yield torch.rand(len(ids), 3, R, R, generator=g) * 2 - 1, torch.ones(len(ids), R, R), ids

    loop = hz.EvalLoop(None, 'cpu', R, N, noise_mode='const', feature_fn=feat, fid_dim=D, latent_fn=lambda ids, b: torch.zeros(b, 4),
                       device_masks=False, step_fn=step, fid_accumulate_fn=acc, fid_real=True)
    loop.run(Loader(loop.ids))
    _, fid = loop.gather()
    assert calls.count('pm1') == calls.count('0_255') == 3
    reals = torch.cat([r for r, _, _ in Loader(list(range(N)))])
    want = (reals.to(torch.float64) * 127.5 + 127.5).reshape(N, -1)[:, :D]
    n, mu, sg = loop.fid_real.mean_cov()
    assert n == N and np.allclose(mu, want.mean(0).numpy(), atol=1e-4)
    fakes = loop.images.to(torch.float64).reshape(N, -1)[:, :D]
    assert np.allclose(fid.mean_cov()[1], fakes.mean(0).numpy())
    assert loop.fid_value() == fid_from_stats(*fid.mean_cov()[1:], *loop.fid_real.mean_cov()[1:])
    plain = hz.EvalLoop(None, 'cpu', R, N, noise_mode='const', feature_fn=feat, fid_dim=D, latent_fn=lambda ids, b: torch.zeros(b, 4),
                        device_masks=False, step_fn=step, fid_accumulate_fn=acc)
    plain.run(Loader(plain.ids))
    _, fid0 = plain.gather()
    assert plain.fid_real is None and torch.equal(fid0.S, fid.S)
    with pytest.raises(ValueError):
        plain.fid_value()
    with pytest.raises(ValueError):
        hz.EvalLoop(None, 'cpu', R, N, fid_real=True)
