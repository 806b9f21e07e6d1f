"""GPU: the device tail of FID (sh-gan_amd/fid_stats.py, csrc/gemm_f64.hip) -- the tiled fp64-MFMA GEMM against numpy float64 under the
textbook bound at sizes on both sides of every tile edge, with pitched views, batches and the diagonal term; ``frechet_device`` against
the eigh yardstick of tests/fid_f64.py at its 21 cases and at the shipped size through ``FidStats``; EvalLoop's ``fid_tail`` option; and the
fill / guard runs of the new allocation sites (they are newer than the site tables of tests/test_gpu_alloc_fill.py /
test_gpu_alloc_guard.py)."""
import numpy as np
import pytest
import torch

import fid_f64 as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -53
SENTINEL = -7.25

# every n of the list: 1 and 3 (less than one MFMA tile), 15 / 16 / 17 and 31 / 33 (the 16-wide MFMA tile and the K chunk of 16), 127 .. 130
# (the 128-wide workgroup tile: one workgroup, then four), 257 and 300 (nine workgroups, ragged chunks)
SIZES = [1, 3, 15, 16, 17, 31, 33, 127, 128, 129, 130, 257, 300]


def _housed(x, pad, fill):
    """numpy [batch, n, n] -> (the whole device buffer [batch, n + 2, n + pad] pre-filled with ``fill``, its view [:, :n, :n] holding x)."""
    batch, n, _ = x.shape
    big = torch.full((batch, n + 2, n + pad), fill, dtype=torch.float64, device=DEV)
    view = big[:, :n, :n]
    view.copy_(torch.from_numpy(x))
    return big, view


@pytest.mark.parametrize('n', SIZES)
def test_gemm_against_float64_under_the_textbook_bound(n):
    """|c - ref| <= (n + 2) 2^-53 (|alpha| |A| |B| + |beta|) at every entry -- n roundings of the products-and-sums in any order, one of the
    scaling, one of the diagonal term -- for pitches n, n + 3 and n + 4 (16-byte and 8-byte loads), batch 1 and 2, (alpha, beta) = (1, 0)
    and (-0.5, 1.5).  Beside the operands lies NaN, beside C a sentinel: a load past a row or below the matrix reaches C, a store outside
    C[:n, :n] changes the sentinel.  The tile partials, added, are tr C and |C|_F^2 to the bound of an n^2-term sum of the entries as
    stored.  Two runs give the same bits."""
    from shgan_amd import fid_stats
    g = np.random.RandomState(n)
    tiles = fid_stats.gemm_f64_tiles(n)
    worst = 0.0
    for pad in (0, 3, 4):
        for batch in (1, 2):
            for alpha, beta in ((1.0, 0.0), (-0.5, 1.5)):
                a, b = g.standard_normal((batch, n, n)), g.standard_normal((batch, n, n))
                (_, da), (_, db) = _housed(a, pad, float('nan')), _housed(b, pad, float('nan'))
                big, dc = _housed(np.zeros((batch, n, n)), pad, SENTINEL)
                dc.fill_(SENTINEL)
                part = torch.full((batch, 2, tiles), float('nan'), dtype=torch.float64, device=DEV)
                if batch == 1:
                    da, db, dc, part = da[0], db[0], dc[0], part[0]
                out = fid_stats.gemm_f64(da, db, alpha=alpha, beta_diag=beta, out=dc, partials=part)
                assert out is dc
                got, sums = big.cpu().numpy().copy(), part.sum(-1).cpu().numpy().reshape(batch, 2)
                part2 = torch.zeros_like(part)
                fid_stats.gemm_f64(da, db, alpha=alpha, beta_diag=beta, out=dc, partials=part2)
                assert torch.equal(big, torch.from_numpy(got).to(DEV)) and torch.equal(part, part2)                  # the same bits on every run
                outside = np.ones(got.shape, bool)
                outside[:, :n, :n] = False
                assert np.all(got[outside] == SENTINEL), 'a store outside C[:n, :n]'
                for k in range(batch):
                    want, bound = ref.gemm_reference(a[k], b[k], alpha, beta)
                    c = got[k, :n, :n]
                    assert np.all(np.isfinite(c)), 'a load outside the operands reached C'
                    worst = max(worst, float(np.max(np.abs(c - want) / bound)))
                    assert np.all(np.abs(c - want) <= bound)
                    # sums of the entries as stored: n (n^2) terms added in some order by the kernel, the tiles by torch.sum
                    assert abs(sums[k, 0] - np.trace(c)) <= (n + tiles + 2) * U * np.abs(np.diag(c)).sum()
                    assert abs(sums[k, 1] - np.sum(c * c)) <= (n * n + tiles + 2) * U * np.sum(c * c)
    print(f'n = {n}: max |c - ref| / bound = {worst:.3e}')


def test_gemm_shared_operand_unaligned_views_and_a_fresh_output():
    """A 2-D operand beside a stack is shared by the batch; a view that starts 8 bytes into a 16-byte pair takes the 8-byte loads and
    gives the bits of the 16-byte loads; ``out=None`` makes the output."""
    from shgan_amd import fid_stats
    n = 130
    g = np.random.RandomState(5)
    a, b = g.standard_normal((n, n)), g.standard_normal((2, n, n))
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    out = fid_stats.gemm_f64(da, db)
    assert out.shape == (2, n, n) and out.is_contiguous()
    for k in range(2):
        want, bound = ref.gemm_reference(a, b[k], 1.0, 0.0)
        assert np.all(np.abs(out[k].cpu().numpy() - want) <= bound)
    assert torch.equal(fid_stats.gemm_f64(db, da)[1], fid_stats.gemm_f64(db[1], da))
    flat = torch.zeros(n * n + 1, dtype=torch.float64, device=DEV)
    shifted = flat[1:].view(n, n)
    shifted.copy_(da)
    assert shifted.data_ptr() % 16 == 8
    assert torch.equal(fid_stats.gemm_f64(shifted, db[0]), out[0]) and torch.equal(fid_stats.gemm_f64(db[1], shifted), fid_stats.gemm_f64(db[1], da))


def test_gemm_refuses_what_it_does_not_serve():
    from shgan_amd import _lib, fid_stats
    x = torch.zeros(8, 8, dtype=torch.float64, device=DEV)
    y = torch.zeros(2, 8, 8, dtype=torch.float64, device=DEV)
    for args, kw in (((x.float(), x), {}), ((x.t(), x), {}), ((x, x[:, :4]), {}), ((x[:4], x), {}), ((x, x), dict(out=x)), ((x, torch.zeros_like(x)), dict(out=x)),
                     ((x, x), dict(out=y)), ((y, x), dict(out=torch.zeros_like(x))), ((y, torch.zeros(3, 8, 8, dtype=torch.float64, device=DEV)), {}),
                     ((x, x), dict(partials=torch.zeros(2, 2, dtype=torch.float64, device=DEV))), ((x, x), dict(partials=torch.zeros(2, 1, device=DEV))),
                     ((x, x), dict(partials=torch.zeros(2, 2, dtype=torch.float64, device=DEV)[:, :1])), ((x.cpu(), x), {}), ((x[::2, ::2], x[:4, :4]), {})):
        with pytest.raises(_lib.ShgError):
            fid_stats.gemm_f64(*args, **kw)


def _device(st):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in st)


@pytest.mark.parametrize('c', ref.CASES)
def test_frechet_device_against_the_eigh_yardstick(c):
    """Relative to tr sigma_f + tr sigma_r (FID itself may be near 0): 1e-7 where N >= 4 D, 1e-5 where N < D (a rank-deficient sigma).
    Worst readings on one MI355X: see MEASUREMENTS.md (FID tail on the device)."""
    from shgan_amd import fid_stats
    D, N = c[:2]
    st = ref.case_stats(*c)
    fid, tr = ref.frechet_eigh(*st)
    scale = float(np.trace(st[1]) + np.trace(st[3]))
    got = fid_stats.frechet_device(*_device(st))
    err = abs(got['fid'] - fid) / scale
    print(f"case {c}: FID {fid:.6f}, |device - eigh| / (tr + tr) = {err:.3e} after {got['iterations']} steps ({got['stop']}, delta {got['delta']:.3e})")
    assert got['stop'] in ('tol', 'turn') and 5 <= got['iterations'] <= 100
    assert err <= ref.bound_of(D, N) and abs(got['trace_sqrt'] - tr) <= ref.bound_of(D, N) * scale
    again = fid_stats.frechet_device(*_device(st))
    assert again == got                                                        # no atomics: the same bits, the same stop


def test_frechet_device_of_identical_sides_is_zero():
    from shgan_amd import fid_stats
    mu, sigma = ref.case_stats(*ref.CASES[9])[:2]
    got = fid_stats.frechet_device(*_device((mu, sigma, mu, sigma)))
    print(f"identical sides: fid {got['fid']:.3e} of 2 tr sigma = {2 * np.trace(sigma):.6f} ({got['iterations']} steps, {got['stop']})")
    assert abs(got['fid']) <= 1e-7 * 2 * np.trace(sigma)


def test_frechet_device_runs_the_gemm_kernel_and_no_blas_gemm():
    import route_probe
    from shgan_amd import fid_stats
    st = _device(ref.case_stats(*ref.CASES[3]))
    got, names = route_probe.launched(lambda: fid_stats.frechet_device(*st), expect=('gemm_f64_kernel',))
    assert got['stop'] in ('tol', 'turn')
    assert route_probe.any_hit('gemm_f64_kernel', names), sorted(names)
    assert not [n for n in names if 'Cijk_' in n], sorted(names)


def test_the_shipped_size_through_fidstats():
    """D = 2048, N = 6000, decay 12, float64 rows through ``FidStats.add`` (dp = 2080) -> ``mean_cov_device`` -> ``frechet_device`` against
    ``frechet_eigh`` of ``mean_cov()`` under the 1e-7 bound (numpy's restatement: 5e-12 in 57 steps).  The one test of this file that takes
    seconds: the host's rotations and eigendecompositions at 2048."""
    from shgan_amd import fid_stats
    D, N = 2048, 6000
    fake, real = ref.features(D, N, 12, 0)
    sides = []
    for x in (fake, real):
        st = fid_stats.FidStats(D, device=DEV)
        assert st.dp == 2080
        for k in range(0, N, 1500):
            st.add(torch.from_numpy(x[k:k + 1500]).to(DEV))
        sides.append(st)
    (n_f, mu_f, sig_f), (n_r, mu_r, sig_r) = (s.mean_cov_device() for s in sides)
    host = sides[0].mean_cov()[1:] + sides[1].mean_cov()[1:]
    assert n_f == n_r == N
    for dev_t, host_t in zip((mu_f, sig_f, mu_r, sig_r), host):
        assert dev_t.is_cuda and dev_t.dtype == torch.float64
        assert np.allclose(dev_t.cpu().numpy(), host_t, rtol=0, atol=4 * U * np.abs(host_t).max() + 4 * U * np.abs(np.outer(host[0], host[0])).max())
    got = fid_stats.frechet_device(mu_f, sig_f, mu_r, sig_r)
    fid, _ = ref.frechet_eigh(*host)
    scale = float(np.trace(host[1]) + np.trace(host[3]))
    print(f"D = 2048: FID {fid:.6f}, |device - eigh| / (tr + tr) = {abs(got['fid'] - fid) / scale:.3e} after {got['iterations']} steps ({got['stop']})")
    assert abs(got['fid'] - fid) <= ref.BOUND_FULL * scale


@pytest.fixture(scope='module')
def small_g():
    from shgan_amd import configs
    G = configs.seeded_init_(configs.build_generator(256, ch_base=2048, ch_max=32, w_dim=64, z_dim=64, w0_dim=128), seed=5, noise_strength=0.1,
                             bias_std=0.1)
    return G.eval().requires_grad_(False).to(DEV)


def _latents(ids, b, z_dim=64):
    out = torch.empty(b, z_dim)
    g = torch.Generator()
    for k, i in enumerate(ids):
        g.manual_seed(500 + int(i))
        out[k].normal_(generator=g)
    return out.to(DEV)


def test_eval_loop_fid_tail(small_g, monkeypatch):
    """256 items (= 4 fid_dim: the full-rank bound), batch 32, random Fourier features of the 8 x 8 pooled image: 'device' is within
    1e-7 (tr + tr) of the same loop's 'host' value and keeps its dict; the default loop calls ``fid_from_stats`` on ``mean_cov`` and returns
    its bits."""
    from shgan_amd import eval_harness as hz, evaluators, fid_stats, kernels
    n_items, b, R, W = 256, 32, 256, 64
    gen = torch.Generator().manual_seed(11)
    proj, phase = (torch.randn(192, W, generator=gen) * 0.7).to(DEV), (torch.rand(W, generator=gen) * 6.283).to(DEV)

    def feats(img, input_range='0_255'):
        if input_range == 'pm1':
            img = (kernels.u8_value_table(DEV)[img.long()] if img.dtype == torch.uint8 else img) * 127.5 + 127.5
        x = torch.nn.functional.adaptive_avg_pool2d(img.float(), 8).flatten(1) / 127.5 - 1.0
        return torch.cos(x @ proj + phase)

    def run(**kw):
        loop = hz.EvalLoop(small_g, DEV, R, n_items, noise_mode='const', depth=2, latent_fn=_latents, feature_fn=feats, fid_dim=W, fid_real=True, **kw)
        np.random.seed(21)
        loop.run(hz.PinnedU8Loader(loop.ids, b, R, seed=13))
        return loop, loop.gather()
    dev, (images, fid) = run(fid_tail='device')
    host, (images0, fid0) = run()
    torch.cuda.synchronize()
    assert torch.equal(images, images0) and torch.equal(fid.S, fid0.S) and torch.equal(dev.fid_real.S, host.fid_real.S)
    calls = []
    monkeypatch.setattr(evaluators, 'fid_from_stats', lambda *a: calls.append(a) or fid_stats.fid_from_stats(*a))
    st = fid0.mean_cov()[1:] + host.fid_real.mean_cov()[1:]
    want = fid_stats.fid_from_stats(*st)
    assert host.fid_value() == want and len(calls) == 1 and host.fid_tail_info is None
    assert all(np.array_equal(x, y) for x, y in zip(calls[0], st))
    got = dev.fid_value()
    info = dev.fid_tail_info
    scale = float(np.trace(st[1]) + np.trace(st[3]))
    print(f"loop: host {want!r}, device {got!r}, |diff| / (tr + tr) = {abs(got - want) / scale:.3e} ({info['iterations']} steps, {info['stop']})")
    assert len(calls) == 1 and got == info['fid'] and info['stop'] in ('tol', 'turn') and info['iterations'] >= 1
    assert abs(got - want) <= ref.BOUND_FULL * scale


def test_new_sites_do_not_depend_on_fresh_contents_and_stay_inside_their_buffers():
    """('fid_stats.py', 'gemm_f64'), ('fid_stats.py', 'mean_cov_device') and ('fid_stats.py', 'frechet_device'): the same bits with every
    fresh allocation pre-filled with NaN bytes and with large values, and no guard band touched with every buffer, the operands included,
    housed between poisoned bands.  n = 130 and 97: ragged tiles whose last loads and stores end at the buffer's last element."""
    import alloc_fill
    import alloc_guard
    from shgan_amd import fid_stats
    sites = {('fid_stats.py', 'gemm_f64'), ('fid_stats.py', 'mean_cov_device'), ('fid_stats.py', 'frechet_device')}
    g = np.random.RandomState(2)
    a, b = g.standard_normal((130, 130)), g.standard_normal((2, 130, 130))
    fake, real = ref.features(97, 400, 6, 0)

    def run():
        da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        tensors = [fid_stats.gemm_f64(da, db, alpha=-0.5, beta_diag=1.5), fid_stats.gemm_f64(da, da)]
        sides = []
        for x in (fake, real):
            st = fid_stats.FidStats(97, device=DEV)
            st.add(torch.from_numpy(x).to(DEV))
            sides.append(st.mean_cov_device(390)[1:])
        tensors += [t for side in sides for t in side]
        return tensors, fid_stats.frechet_device(*sides[0], *sides[1])
    want, want_d = run()
    torch.cuda.synchronize()
    for pattern in ('nan', 'big'):
        with alloc_fill.filled(pattern) as rec:
            got, got_d = run()
            torch.cuda.synchronize()
        assert sites <= rec.sites, rec.sites
        assert got_d == want_d and all(torch.equal(x, y) for x, y in zip(got, want)), pattern
    with alloc_guard.guarded() as rec:
        got, got_d = run()
        bad = rec.violations()
        assert sites <= rec.sites and not bad, bad
        assert got_d == want_d and all(torch.equal(x, y) for x, y in zip(got, want))
