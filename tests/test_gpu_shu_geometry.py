"""GPU: the Spectral Hint Unit at input sizes 16 .. 128 and any lowest level (csrc/shu.hip, the ``*_n_kernel`` templates) against the
reference's SHU (tests/golden/shu_geometry*.npz, written by tools/gen_golden_shu_geometry.py), the CPU oracle and torch.fft in float64.

Cases (all tail_sigma_mult = 3, conv0.bias ~ N(0, 0.2)):
  A  N=2 C=32 input 32  lowest 4    fused spectral stage with a partial last tile (544 positions), 4 levels
  B  N=1 C=32 input 128 lowest 8    fused at 128, levels 64 and 128 on the matrix cores, Gaussian on the top level
  C  N=2 C=8  input 16  lowest 16   one level, bicubic [3,2] bands, unfused route with 144 positions
  D  N=2 C=16 input 64  lowest 16   shipped size, shorter pyramid, 2C != 64
  E  N=1 C=12 input 128 lowest 4    six levels, channel count no multiple of 8
  G  a 256^2 generator whose SHU reads the 32^2 feature and stops at 8
The reference's float32 is within 1.5e-7 of its float64 at every level of A-E; the bounds below are those of the existing SHU tests."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from route_probe import any_hit, launched
from test_shu_geometry_cpu import build_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4                     # test_shu_golden
N_KERNELS = ('shu_rfft2_shift_n_kernel', 'shu_split_irfft2_n_kernel', 'shu_split_adjoint_n_kernel', 'shu_spectral_tail_kernel')


def c(a):
    return a.detach().cpu().numpy()


@pytest.fixture(scope='module')
def cases():
    """Per case: the unit on the device, its input, the fixture and the reference hints (levels >= 64: the stored channels only)."""
    out = {}
    for cid in 'ABCDE':
        shu, g, (n, ch, size, lowest, seed) = build_case(cid)
        x = np.random.RandomState(seed).standard_normal((n, ch, size, size)).astype(np.float32)
        keep = [int(v) for v in g[f'{cid}__channels']]
        out[cid] = dict(shu=shu.to(DEV).eval().requires_grad_(False), x=x, keep=keep, size=size, lowest=lowest, ch=ch, n=n,
                        ref={r: g[f'{cid}__y{r}'] for r in shu.reslist})
    return out


def stored(case, r, t):
    return t[:, case['keep']] if r >= 64 else t


@pytest.mark.parametrize('cid', list('ABCDE'))
def test_forward_matches_the_reference(cases, cid):
    from oracle import shgan_oracle as orc
    k = cases[cid]
    shu = k['shu']
    out = shu(torch.from_numpy(k['x']).to(DEV))
    assert sorted(out) == shu.reslist
    for r in shu.reslist:
        assert tuple(out[r].shape) == (k['n'], k['ch'], r, r)
        e = rel_err(stored(k, r, c(out[r])), k['ref'][r])
        print(f'case {cid} level {r}: rel_err vs reference {e:.3e}')
        assert e < TOL, (cid, r, e)
    if cid in 'ADE':     # the oracle's shu_forward takes input_res / lowest_res, with [2,3] piecewise-linear bands and a flat top level only
        sd = {key: v.detach().cpu() for key, v in shu.state_dict().items()}
        ref = orc.shu_forward(sd, torch.from_numpy(k['x']), p='', input_res=k['size'], lowest_res=k['lowest'])
        for r in shu.reslist:
            e = rel_err(c(out[r]), ref[r].numpy())
            print(f'case {cid} level {r}: rel_err vs oracle {e:.3e}')
            assert e < TOL, (cid, r, e)


@pytest.mark.parametrize('size', [16, 32, 64, 128])
def test_spectrum_alone_against_torch_fft(size):
    from shgan_amd import kernels
    x = np.random.RandomState(size).standard_normal((2, 3, size, size)).astype(np.float32)
    xb = torch.zeros(2, 5, size, size, device=DEV)
    xb[:, 2:] = torch.from_numpy(x).to(DEV)
    t = c(kernels.shu_rfft2_shift(xb[:, 2:]))                      # a channel slice: planes contiguous, batch stride of the wider tensor
    assert t.shape == (2, 6, size, size // 2 + 1)
    sp = torch.fft.rfftn(torch.from_numpy(x), dim=(2, 3), norm='forward')
    sp = torch.cat([sp[:, :, size // 2 + 1:], sp[:, :, :size // 2 + 1]], dim=2)
    er, ei = rel_err(t[:, :3], sp.real.numpy()), rel_err(t[:, 3:], sp.imag.numpy())
    print(f'spectrum {size}: rel_err re {er:.3e} im {ei:.3e}')
    assert er < 1e-5 and ei < 1e-5


@pytest.mark.parametrize('cid', list('ABC'))
def test_accumulate_form_writes_only_its_channel_slice(cases, cid):
    k = cases[cid]
    shu = k['shu']
    feats = {r: torch.zeros(k['n'], k['ch'] + 8, r, r, device=DEV) for r in shu.reslist}
    shu.forward_accumulate(torch.from_numpy(k['x']).to(DEV), feats)
    for r in shu.reslist:
        assert rel_err(stored(k, r, c(feats[r][:, 8:])), k['ref'][r]) < TOL, (cid, r)
        assert float(feats[r][:, :8].abs().max()) == 0.0, (cid, r)
    shu.forward_accumulate(torch.from_numpy(k['x']).to(DEV), feats)                   # and it adds
    for r in shu.reslist:
        assert rel_err(stored(k, r, c(feats[r][:, 8:])), 2 * k['ref'][r]) < TOL, (cid, r)


@pytest.mark.parametrize('cid', list('AB'))
def test_fused_spectral_stage_vs_two_convolutions(cases, cid):
    from shgan_amd.model_zoo import shgan
    k = cases[cid]
    shu, x = k['shu'], torch.from_numpy(k['x']).to(DEV)
    old = shgan.SHU.FUSED_SPECTRAL
    try:
        shgan.SHU.FUSED_SPECTRAL = True
        a, names = launched(lambda: shu(x), expect=['shu_spectral'])
        shgan.SHU.FUSED_SPECTRAL = False
        b, names_b = launched(lambda: shu(x))
    finally:
        shgan.SHU.FUSED_SPECTRAL = old
    assert any_hit('shu_spectral_tail_kernel' if cid == 'A' else 'shu_spectral_kernel', names), names
    assert not any_hit('shu_spectral_kernel', names_b) and not any_hit('shu_spectral_tail_kernel', names_b), names_b
    for r in shu.reslist:
        assert not torch.equal(a[r], b[r])
        e = rel_err(c(a[r]), c(b[r]))
        print(f'case {cid} level {r}: fused vs unfused {e:.3e}')
        assert e < 2e-5, (cid, r, e)


def fft_form(shu, x, params, gauss, cw):
    """shgan.py:312-336 with torch.fft at the unit's geometry, in the dtype of ``x``."""
    w0, b0, w1 = params
    size, half = shu.input_res, shu.input_res // 2
    sp = torch.fft.rfftn(x, dim=(2, 3), norm='forward')
    sp = torch.cat([sp[:, :, half + 1:], sp[:, :, :half + 1]], dim=2)
    t = torch.cat([sp.real, sp.imag], dim=1)
    t = torch.relu(torch.nn.functional.conv2d(t, w0 * shu.conv0.weight_gain, b0))
    y = torch.nn.functional.conv2d(t, w1.t()[:, :, None, None])             # df1.weight is [in, out * bands]; flat output channel = o * bands + k
    y = (y.reshape(y.shape[0], -1, cw.shape[0], size, half + 1) * cw[None, None]).sum(2)
    ch = y.shape[1] // 2
    sp = torch.complex(y[:, :ch], y[:, ch:])
    out = {}
    for r in shu.reslist:
        s_ = sp[:, :, half - r // 2: half + r // 2, 0: r // 2 + 1] * gauss[r][None, None]
        s_ = torch.cat([s_[:, :, r - r // 2 - 1:], s_[:, :, :r - r // 2 - 1]], dim=2)
        out[r] = torch.fft.irfftn(s_, dim=(2, 3), norm='forward')
    return out


def f64_setup(shu, x0):
    xr = torch.tensor(x0, dtype=torch.float64, requires_grad=True)
    pr = [p.detach().cpu().double().requires_grad_(True) for p in (shu.conv0.weight, shu.conv0.bias, shu.df1.weight)]
    gauss = {r: getattr(shu, f'_gauss{r}').cpu().double() for r in shu.reslist}
    return xr, pr, gauss, shu._cw.cpu().double()


@pytest.mark.parametrize('cid', list('ACE'))
def test_training_route_matches_the_fft_formulation(cases, cid):
    """Hints and the gradients of a random functional w.r.t. the input and the parameters against float64 torch.fft on the CPU (bounds of
    test_shu_training_route_matches_the_fft_formulation: 2e-5 / 5e-5); the adjoint kernel runs, no rocFFT / rocBLAS kernel does."""
    from torch.profiler import ProfilerActivity, profile
    k = cases[cid]
    shu, x0 = k['shu'], k['x'].astype(np.float64)
    rs = np.random.RandomState(77)
    ws = {r: rs.standard_normal((k['n'], k['ch'], r, r)) for r in shu.reslist}
    with torch.enable_grad():
        xr, pr, gauss, cw = f64_setup(shu, x0)
        ref = fft_form(shu, xr, pr, gauss, cw)
        gref = torch.autograd.grad(sum((ref[r] * torch.tensor(ws[r])).sum() for r in shu.reslist), [xr] + pr)
        shu.requires_grad_(True)
        try:
            xg = torch.tensor(x0, dtype=torch.float32, device=DEV, requires_grad=True)
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                got = shu(xg)
                loss_g = sum((got[r] * torch.tensor(ws[r], dtype=torch.float32, device=DEV)).sum() for r in shu.reslist)
                ggot = torch.autograd.grad(loss_g, [xg, shu.conv0.weight, shu.conv0.bias, shu.df1.weight])
                torch.cuda.synchronize()
        finally:
            shu.requires_grad_(False)
    for r in shu.reslist:
        e = float((got[r].detach().cpu().double() - ref[r].detach()).abs().max() / ref[r].detach().abs().max())
        print(f'case {cid} level {r}: training hints vs float64 {e:.3e}')
        assert e < 2e-5, (cid, r, e)
    for name, a, b in zip(('x', 'conv0.weight', 'conv0.bias', 'df1.weight'), ggot, gref):
        e = float((a.detach().cpu().double() - b).abs().max() / b.abs().max())
        print(f'case {cid} grad {name}: vs float64 {e:.3e}')
        assert e < 5e-5, (cid, name, e)
    names = [e.key for e in prof.key_averages()]
    assert any('shu_split_adjoint_n_kernel' in n for n in names), names
    assert not any(n.startswith('Cijk_') or ('fft' in n.lower() and 'shu_' not in n) for n in names), names       # (rocBLAS / rocFFT kernel names)


def test_second_order_smoke_at_the_one_level_case(cases):
    """Gradient w.r.t. x of the squared norm of dL/dx, L = sum w * hint^2 / 2 (a functional whose first gradient still depends on x),
    at case C against float64: the transposes of the two transform stages are differentiable again."""
    k = cases['C']
    shu, x0 = k['shu'], k['x'].astype(np.float64)
    w = np.random.RandomState(78).standard_normal((k['n'], k['ch'], 16, 16))

    def second(x, hints, wt):
        (gx,) = torch.autograd.grad((hints[16].square() * wt).sum() * 0.5, x, create_graph=True)
        (ggx,) = torch.autograd.grad(gx.square().sum(), x)
        return ggx

    with torch.enable_grad():
        xr, pr, gauss, cw = f64_setup(shu, x0)
        want = second(xr, fft_form(shu, xr, pr, gauss, cw), torch.tensor(w))
        shu.requires_grad_(True)
        try:
            xg = torch.tensor(x0, dtype=torch.float32, device=DEV, requires_grad=True)
            got = second(xg, shu(xg), torch.tensor(w, dtype=torch.float32, device=DEV))
        finally:
            shu.requires_grad_(False)
    e = float((got.cpu().double() - want).abs().max() / want.abs().max())
    print(f'case C second order: vs float64 {e:.3e}')
    assert e < 5e-5, e


def test_generator_with_a_32_to_8_unit_matches_the_reference():
    """Case G: image and the hinted skip features against the reference's Generator (bounds of test_generator_small_golden); known-region
    pixels of the uint8 composite bit-exact."""
    from oracle import shgan_oracle as orc
    from shgan_amd import configs, eval_harness, kernels
    g = load_golden('shu_geometry_g')
    res, ch_base, ch_max, w_dim, z_dim, w0_dim = [int(v) for v in g['cfg']]
    seed = int(g['seed'])
    G = configs.build_generator(res, ch_base=ch_base, ch_max=ch_max, w_dim=w_dim, z_dim=z_dim, w0_dim=w0_dim,
                                shu=dict(shu_input_res=int(g['shu_input_res']), shu_lowest_res=int(g['shu_lowest_res'])))
    G.load_state_dict(orc.init_state_dict(res, seed=seed, ch_base=ch_base, ch_max=ch_max, w_dim=w_dim, z_dim=z_dim, w0_dim=w0_dim,
                                          noise_strength=0.1, bias_std=0.1), strict=True)
    G = G.eval().requires_grad_(False).to(DEV)
    rs = np.random.RandomState(seed + 1)                                                  # the generator tool's draws, in its order
    real_u8 = rs.randint(0, 256, size=(1, 3, res, res)).astype(np.uint8)
    z = torch.from_numpy(rs.standard_normal((1, z_dim)).astype(np.float32)).to(DEV)
    mask = torch.from_numpy(np.unpackbits(g['mask_bits'])[: res * res].reshape(1, 1, res, res).astype(np.float32))
    x = eval_harness.assemble_input(torch.from_numpy(real_u8.astype(np.float32)) / 127.5 - 1.0, mask).to(DEV)
    (img, feats), names = launched(lambda: (G(x=x, z=z, c=torch.zeros(1, 0, device=DEV), noise_mode='const'), G.encoder(x)[1]),
                                   expect=['shu_rfft2_shift_n_kernel<32>'])
    assert any_hit('shu_rfft2_shift_n_kernel<32>', names) and any_hit('shu_split_irfft2_n_kernel<32>', names), names
    for r in (8, 16, 32):
        assert rel_err(c(feats[r]), g[f'feat{r}']) < 1e-4, r
    e = rel_err(c(img), g['img_const'])
    print(f'case G image: rel_err {e:.3e}')
    assert e < 1e-3
    u8 = kernels.composite_u8(x, img)
    known = (u8.cpu() * mask.to(torch.uint8)).numpy()
    assert hashlib.sha256(known.tobytes()).hexdigest() == str(g['known_sha256'])


def test_shipped_geometry_keeps_its_kernels_and_its_result():
    from oracle import shgan_oracle as orc
    from shgan_amd.model_zoo import shgan
    gd = load_golden('shu')
    sd = orc.init_state_dict(256, seed=int(gd['shu__seed']), ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128, bias_std=0.2)
    shu = shgan.SHU(32, 32, [2, 3], 'piecewise_linear', 64, 4)
    shu.load_state_dict({k[len('encoder.shu.'):]: v for k, v in sd.items() if k.startswith('encoder.shu.')}, strict=True)
    shu = shu.to(DEV).eval()
    x = torch.from_numpy(gd['shu__x']).to(DEV)
    shipped = ['shu_rfft2_shift_kernel', 'shu_spectral_kernel', 'shu_split_irfft2_kernel']
    out, names = launched(lambda: shu(x), expect=shipped)
    for p in shipped:
        assert any_hit(p, names), (p, names)
    for p in N_KERNELS:
        assert not any_hit(p, names), (p, names)
    for r in (4, 8, 16, 32, 64):
        assert rel_err(c(out[r]), gd[f'shu__y{r}']) < TOL, r
